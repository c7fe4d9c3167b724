"""Colour control in fp64 numpy: the yardstick of csrc/color.hip and
styletransfer_amd/color.py (the reference project has no such feature).

Images are [3][h][w] (or [n][3][h][w] for `stats`) fp64 arrays in the ImageNet-normalised
space of the package's tensors.  Everything is written from the definitions -- moments by
numpy means, matrix square roots by eigh, the affine map by einsum -- so that it shares
no arithmetic with the code under test."""
import numpy as np

W = np.array([0.299, 0.587, 0.114])
MEAN = np.array([0.485, 0.456, 0.406])
STD = np.array([0.229, 0.224, 0.225])
TRI = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]


def stats(x):
    """[.., 3, h, w] -> [.., 9]: mean[3], population covariance upper triangle."""
    x = np.asarray(x, np.float64)
    if x.ndim == 4:
        return np.stack([stats(i) for i in x])
    p = x.reshape(3, -1)
    mu = p.mean(axis=1)
    d = p - mu[:, None]
    cov = d @ d.T / p.shape[1]
    return np.concatenate([mu, [cov[a, b] for a, b in TRI]])


def mu_cov(s):
    s = np.asarray(s, np.float64)
    cov = np.zeros((3, 3))
    for v, (a, b) in zip(s[3:], TRI):
        cov[a, b] = cov[b, a] = v
    return s[:3], cov


def sym_power(cov, p, floor=0.0):
    lam, vec = np.linalg.eigh(cov)
    lam = np.maximum(lam, floor)
    return vec @ np.diag(lam ** p) @ vec.T


def eig_floor(cov):
    return max(1e-6 * np.trace(cov), 1e-12)


def match_matrix(stats_style, stats_content):
    mu_s, cov_s = mu_cov(stats_style)
    mu_c, cov_c = mu_cov(stats_content)
    A = sym_power(cov_c, 0.5) @ sym_power(cov_s, -0.5, eig_floor(cov_s))
    return A, mu_c - A @ mu_s


def affine(x, M, b=None, base=None, lo=None, hi=None):
    """out[c] = clamp(base[c] + sum_d M[c][d] (x[d] - base[d]) + b[c]) on [.., 3, h, w]."""
    x = np.asarray(x, np.float64)
    M = np.asarray(M, np.float64)
    sh = (3, 1, 1)
    t = x if base is None else x - base
    out = np.einsum("cd,...dhw->...chw", M, t)
    if b is not None:
        out = out + np.asarray(b, np.float64).reshape(sh)
    if base is not None:
        out = out + base
    if lo is not None:
        out = np.minimum(np.maximum(out, np.asarray(lo, np.float64).reshape(sh)),
                         np.asarray(hi, np.float64).reshape(sh))
    return out


def match(style, content):
    """The style image recoloured to the content's mean and covariance."""
    return affine(style, *match_matrix(stats(style), stats(content)))


def denorm(x):
    return np.asarray(x, np.float64) * STD.reshape(3, 1, 1) + MEAN.reshape(3, 1, 1)


def renorm(p):
    return (p - MEAN.reshape(3, 1, 1)) / STD.reshape(3, 1, 1)


def luma_of(x):
    """De-normalised luminance plane [h][w] of a normalised image."""
    return np.einsum("d,dhw->hw", W, denorm(x))


def luma_moments(s):
    mu, cov = mu_cov(s)
    ws = W * STD
    return W @ (mu * STD + MEAN), ws @ cov @ ws


def luma_gain(stats_style, stats_content):
    ms, vs = luma_moments(stats_style)
    mc, vc = luma_moments(stats_content)
    a = np.sqrt(max(vc, 0.0) / vs) if vs > 1e-12 else 1.0
    return a, mc - a * ms


def luma_matrix(a=1.0, o=0.0):
    M = np.array([[a * W[d] * STD[d] / STD[c] for d in range(3)] for c in range(3)])
    b = np.array([(a * (W @ MEAN) + o - MEAN[c]) / STD[c] for c in range(3)])
    return M, b


def luminance(x, a=1.0, o=0.0):
    """The luminance image (R = G = B = a Y + o after de-normalising), normalised."""
    y = a * luma_of(x) + o
    return renorm(np.stack([y, y, y]))


def merge_matrix():
    return np.array([[W[d] * STD[d] / STD[c] for d in range(3)] for c in range(3)])


def gamut_bounds():
    return (0.0 - MEAN) / STD, (1.0 - MEAN) / STD


def merge(stylised, content, clamp=False):
    """The stylised image's luminance with the content's chroma: every de-normalised
    channel of the content moves by the luminance difference."""
    d = luma_of(stylised) - luma_of(content)
    out = renorm(denorm(content) + d[None])
    if clamp:
        lo, hi = gamut_bounds()
        out = np.minimum(np.maximum(out, lo.reshape(3, 1, 1)), hi.reshape(3, 1, 1))
    return out


# Rec.601 / NTSC RGB -> YIQ, for the independent route of the merge identity
RGB2YIQ = np.array([[0.299, 0.587, 0.114],
                    [0.595716, -0.274453, -0.321263],
                    [0.211456, -0.522591, 0.311135]])


def yiq(x):
    """[3][h][w] normalised image -> its de-normalised Y, I, Q planes."""
    return np.einsum("cd,dhw->chw", RGB2YIQ, denorm(x))


def merge_by_yiq(stylised, content):
    """Y from the stylised image, I and Q from the content, inverted with numpy."""
    ys, yc = yiq(stylised), yiq(content)
    mixed = np.stack([ys[0], yc[1], yc[2]])
    return renorm(np.einsum("cd,dhw->chw", np.linalg.inv(RGB2YIQ), mixed))
