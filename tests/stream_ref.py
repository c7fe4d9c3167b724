"""Plain fp64 CPU references of the HBM-bound libstx kernels (elementwise.hip, vec.hip,
the gradient-stats pair of lbfgs.hip, stx_loss_finalize), one short function per
operation, each written from include/stx.h's statement of the op and not from the kernel.
tests/test_stream_ref_host.py pins them against torch fp64 autograd;
tests/test_streaming_gpu.py compares the kernels with them element by element.

Inputs are numpy arrays of any float dtype (read as float64).  A reduction returns
(value, sum of the magnitudes of its terms): the second is what its error bound scales
with.  NaN is ordinary data and propagates the way the header says it does."""
import numpy as np
import torch

NAN = float("nan")


def f64(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def relu(x):
    """max(x, 0) with NaN kept (torch.relu)."""
    x = f64(x)
    return np.where(x <= 0, 0.0, x)


# ----------------------------------------------------------------------- losses
def sqdiff(a, b, relu_inputs=False):
    """s = sum((f(a) - f(b))^2); its terms are non-negative, so sum|terms| = s."""
    a, b = f64(a).ravel(), f64(b).ravel()
    if relu_inputs:
        a, b = relu(a), relu(b)
    return float(np.sum((a - b) ** 2))


def mse(a, b, mode, relu_inputs=False):
    """stx_mse's out for mode 0 / 1 / 2, as an fp64 vector of 1 / 2 / 3 values."""
    n = f64(a).size
    if mode == 0:
        return np.array([sqdiff(a, b, relu_inputs) / n])
    if mode == 1:
        mean = sqdiff(a, b, relu_inputs) / n
        return np.array([mean * mean / n, mean])
    mr = sqdiff(a, b, True) / n
    return np.array([sqdiff(a, b, False) / n, mr * mr / n, mr])


def mse_grad(a, b, gscale):
    """grad = gscale * 2 (a - b) / n  (mode 0); also the magnitude sum of its two terms."""
    a, b = f64(a), f64(b)
    s = gscale * 2.0 / a.size
    return s * (a - b), abs(s) * (np.abs(a) + np.abs(b))


def diff_scale(a, b, s0, s1=None, s2=None, relu_inputs=False, old=None):
    """grad (+)= s0 s1 s2 (f(a) - f(b)) [(a > 0) if relu]; (value, magnitude sum)."""
    a, b = f64(a), f64(b)
    sc = float(s0) * (1.0 if s1 is None else float(s1)) * (1.0 if s2 is None else float(s2))
    fa, fb = (relu(a), relu(b)) if relu_inputs else (a, b)
    mask = (a > 0).astype(np.float64) if relu_inputs else 1.0
    v = sc * (fa - fb) * mask
    mag = abs(sc) * (np.abs(fa) + np.abs(fb)) * mask
    if old is not None:
        v, mag = v + f64(old), mag + np.abs(f64(old))
    return v, mag


def loss_combine(s, w):
    """sum_i w[i] s[i]; (value, sum|terms|)."""
    t = f64(w) * f64(s)[:len(w)]
    return float(np.sum(t)), float(np.sum(np.abs(t)))


def loss_finalize(parts, inv, extra=(), w=None):
    """losses[i] = inv[i] sum(parts[i]); total = sum w[i] losses[i] + sum w[k+j] extra[j].
    Returns (losses, sum|terms| per loss, total, sum|terms| of total); the last two are
    None without w."""
    losses = np.array([float(iv) * np.sum(f64(p)) for p, iv in zip(parts, inv)])
    mags = np.array([abs(float(iv)) * np.sum(np.abs(f64(p))) for p, iv in zip(parts, inv)])
    if w is None:
        return losses, mags, None, None
    t = f64(w) * np.concatenate([losses, f64(extra).ravel()])
    return losses, mags, float(np.sum(t)), float(np.sum(np.abs(t)))


# ----------------------------------------------------------------------- pooling / relu
def maxpool_fwd(x, relu_input=False):
    """MaxPool2d(2, 2), floor mode, over [nc][h][w]: values and the flat y*w+x index of the
    first maximum in row-major window order; a NaN wins (the last one in the window, as
    torch's CPU kernel updates on `v > max or isnan(v)`)."""
    x = f64(x)
    if relu_input:
        x = relu(x)
    nc, h, w = x.shape
    ho, wo = h // 2, w // 2
    best = np.full((nc, ho, wo), -np.inf)
    idx = np.zeros((nc, ho, wo), dtype=np.int64)
    oy, ox = np.meshgrid(np.arange(ho), np.arange(wo), indexing="ij")
    idx[:] = (2 * oy) * w + 2 * ox
    for dy in range(2):
        for dx in range(2):
            v = x[:, dy:2 * ho:2, dx:2 * wo:2]
            take = (v > best) | np.isnan(v)
            best = np.where(take, v, best)
            idx = np.where(take, (2 * oy + dy) * w + 2 * ox + dx, idx)
    return best, idx


def maxpool_bwd(dy, idx, h, w):
    """dx = scatter(dy at idx): every input element not an argmax, and the trailing row /
    column of an odd plane, gets 0."""
    dy = f64(dy)
    nc, k = dy.shape[0], dy.shape[1] * dy.shape[2]
    dx = np.zeros((nc, h * w))
    np.put_along_axis(dx, np.asarray(idx).reshape(nc, k), dy.reshape(nc, k), axis=1)
    return dx.reshape(nc, h, w)


def relupool_bwd(dp, z):
    """dz = unpool(dp) * (z > 0), the argmax that of maxpool(relu(z)).  A NaN z is not
    positive: 0 there (torch's backward of ReLU + MaxPool2d gives the same)."""
    z = f64(z)
    _, idx = maxpool_fwd(z, relu_input=True)
    return np.where(z > 0, maxpool_bwd(dp, idx, z.shape[1], z.shape[2]), 0.0)


def relu_bwd(dy, y):
    """dx = dy * (y > 0)  (0 at a NaN y, as torch's threshold backward)."""
    return np.where(f64(y) > 0, f64(dy), 0.0)


# ----------------------------------------------------------------------- upsample / tv
def upsample_fwd(x):
    return np.repeat(np.repeat(f64(x), 2, axis=-2), 2, axis=-1)


def upsample_bwd(dy):
    """dx = the sum of dy's 2x2 block; (value, magnitude sum)."""
    dy = f64(dy)
    nc, H, W = dy.shape
    b = dy.reshape(nc, H // 2, 2, W // 2, 2)
    return b.sum(axis=(2, 4)), np.abs(b).sum(axis=(2, 4))


def tv(y, factor, gscale=1.0, gscale_dev=None):
    """Total variation, batch sum, of y [n][c][h][w]: (loss, sum|terms| of the loss,
    grad = gscale gscale_dev d loss / dy, magnitude sum of grad's sign terms)."""
    y = f64(y)
    dh = y[..., :, :-1] - y[..., :, 1:]
    dv = y[..., :-1, :] - y[..., 1:, :]
    s = float(np.sum(np.abs(dh)) + np.sum(np.abs(dv)))
    g = np.zeros_like(y)
    cnt = np.zeros_like(y)
    for d, lo, hi in ((dh, np.s_[..., :, :-1], np.s_[..., :, 1:]),
                      (dv, np.s_[..., :-1, :], np.s_[..., 1:, :])):
        g[lo] += np.sign(d)
        g[hi] -= np.sign(d)
        cnt[lo] += np.abs(np.sign(d))
        cnt[hi] += np.abs(np.sign(d))
    gs = factor * gscale * (1.0 if gscale_dev is None else float(gscale_dev))
    return factor * s, abs(factor) * s, gs * g, abs(gs) * cnt


# ----------------------------------------------------------------------- bias grad
def bias_grad(dy, old=None):
    """db[c] (+)= sum_{n,p} dy[n][c][p] over dy [n][c][hw]; (value, sum|terms|)."""
    dy = f64(dy)
    v, mag = dy.sum(axis=(0, 2)), np.abs(dy).sum(axis=(0, 2))
    if old is not None:
        v, mag = v + f64(old), mag + np.abs(f64(old))
    return v, mag


# ----------------------------------------------------------------------- vectors
def vec_reduce(a, b, op, mul=None, add=None, sgn=1.0):
    """r = dot(a, b) (0), sum|a| (1), max|a| (2, NaN propagates; 0 for n = 0), then
    out = add + sgn r mul.  Returns (out, sum of magnitudes of everything added)."""
    a = f64(a).ravel()
    if op == 0:
        t = a * f64(b).ravel()
        r, mag = float(np.sum(t)), float(np.sum(np.abs(t)))
    elif op == 1:
        r = mag = float(np.sum(np.abs(a)))
    else:
        r = mag = (NAN if np.isnan(a).any() else float(np.max(np.abs(a)))) if a.size else 0.0
    mu = 1.0 if mul is None else float(mul)
    ad = 0.0 if add is None else float(add)
    return ad + sgn * r * mu, abs(ad) + mag * abs(mu)


def axpby(y, x, a, b, a_dev=None, a_sgn=1.0):
    """y = alpha x + b y, alpha = a_sgn a_dev a with a_dev, else a; x None: y = b y.  b == 0
    does not read y.  (value, magnitude sum)."""
    alpha = float(a) if a_dev is None else a_sgn * float(a_dev) * float(a)
    y = f64(y)
    by = np.zeros_like(y) if b == 0 else b * y
    ax = np.zeros_like(y) if x is None else alpha * f64(x)
    return ax + by, np.abs(ax) + np.abs(by)


def scalar_op(s, op, i, j, k):
    """s[k] = s[i] op s[j]: 0 div, 1 mul, 2 sub, 3 add, 4 1/s[i], 5 min(s[j], 1/s[i]).
    Returns the new array and the magnitude sum of s[k]'s terms."""
    s = f64(s).copy()
    a, b = s[i], (s[j] if j >= 0 else 0.0)
    if op == 0:
        r = a / b
    elif op == 1:
        r = a * b
    elif op == 2:
        r = a - b
    elif op == 3:
        r = a + b
    elif op == 4:
        r = 1.0 / a
    else:
        r = min(b, 1.0 / a)
    s[k] = r
    return s, (abs(a) + abs(b) if op in (2, 3) else abs(r))


def grad_stats(g, loss=None):
    """(loss or None, max|g| with NaN propagating, sum|g|)."""
    g = f64(g).ravel()
    mx = NAN if np.isnan(g).any() else float(np.max(np.abs(g)))
    return (None if loss is None else float(loss)), mx, float(np.sum(np.abs(g)))


# ----------------------------------------------------------------------- Adam
def adam(p, g, m, v, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """Step number t (1-based) of torch.optim.Adam in fp64 from the state (p, m, v) after
    t - 1 steps; returns the new (p, m, v)."""
    pt = torch.tensor(f64(p).copy(), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([pt], lr=lr, betas=(b1, b2), eps=eps)
    opt.state[pt] = {"step": torch.tensor(float(t - 1)),
                     "exp_avg": torch.tensor(f64(m).copy()),
                     "exp_avg_sq": torch.tensor(f64(v).copy())}
    pt.grad = torch.tensor(f64(g).copy())
    opt.step()
    st = opt.state[pt]
    return pt.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()
