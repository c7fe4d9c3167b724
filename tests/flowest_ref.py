"""Test helper (not a test module): numpy restatement of the optical-flow estimator as
include/stx.h defines it -- coarse-to-fine Horn-Schunck with warping,
relaxed by Jacobi iterations -- with the dtype as a parameter.

dtype = np.float64 is the yardstick.  dtype = np.float32 follows the header's operation
order: every product, sum and division rounds to fp32 where the header's expression does,
and an fmaf is the exactly formed product plus the addend rounded once (formed in fp64,
where the product of two fp32 values is exact, and rounded to fp32: equal to a hardware fmaf
except in rare double-rounding ties).  It is what "fp32's own error against fp64" means in
tests/test_flowest_gpu.py.

Also the test clips: textured frame pairs whose true flow is exact by construction."""
import functools

import numpy as np

import flow_ref
import scale_ref

MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)


def _fma(a, b, c, dt):
    if dt == np.float32:
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64)
                + np.asarray(c, np.float64)).astype(np.float32)
    return a * b + c


def pyramid(h, w, min_side=16):
    """[(h_0, w_0), ...], finest first: a level is added while min(h_l, w_l) // 2 >= min_side."""
    levels = [(h, w)]
    while min(h, w) // 2 >= min_side:
        h, w = -(-h // 2), -(-w // 2)
        levels.append((h, w))
    return levels


def luma(img, mean=MEAN, std=STD, dtype=np.float64):
    """[n][h][w]: 255 (0.299 R + 0.587 G + 0.114 B), R = r std_r + mean_r (mean and std are
    the fp32 values the kernel receives)."""
    dt = dtype
    x = np.asarray(img, np.float32).astype(dt)
    m, s = np.asarray(mean, np.float32).astype(dt), np.asarray(std, np.float32).astype(dt)
    R, G, B = (_fma(x[:, k], s[k], m[k], dt) for k in range(3))
    l = dt(0.299) * R
    l = _fma(dt(0.587), G, l, dt)
    l = _fma(dt(0.114), B, l, dt)
    return dt(255.0) * l


def _resize_axis(x, n_out, axis, dt):
    n_in = x.shape[axis]
    if n_in == n_out:
        return x
    first, count, w, k = scale_ref.plan(n_in, n_out, "triangle")
    w = w.astype(np.float32).astype(dt) if dt == np.float32 else w
    x = np.moveaxis(x, axis, -1)
    acc = None
    for t in range(k):
        idx = np.minimum(first + t, n_in - 1)  # (past the count the weight is 0)
        acc = w[:, t] * x[..., idx] if acc is None else _fma(w[:, t], x[..., idx], acc, dt)
    return np.moveaxis(acc, -1, axis)


def resize(x, ho, wo, dtype=np.float64):
    """stx_resample2d, triangle: horizontal, then vertical; each output an fmaf chain over
    its taps in ascending order from w0 x0 (weights formed in fp64, for fp32 rounded once)."""
    x = np.asarray(x).astype(dtype)
    return _resize_axis(_resize_axis(x, wo, -1, dtype), ho, -2, dtype)


def _taps(flow, dt):
    n, _, h, w = flow.shape
    u, v = flow[:, 0], flow[:, 1]
    ii = np.arange(h, dtype=dt)[None, :, None]
    jj = np.arange(w, dtype=dt)[None, None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        y = np.fmin(np.fmax(ii + v, dt(0)), dt(h - 1))  # fmax / fmin: a NaN becomes 0
        x = np.fmin(np.fmax(jj + u, dt(0)), dt(w - 1))
    y0 = np.minimum(np.floor(y), h - 2).astype(np.int64)
    x0 = np.minimum(np.floor(x), w - 2).astype(np.int64)
    fy, fx = y - y0.astype(dt), x - x0.astype(dt)
    gy, gx = dt(1) - fy, dt(1) - fx
    return y0, x0, (gy * gx, gy * fx, fy * gx, fy * fx)


def _sample(P, y0, x0, wts, dt, want_mag=False):
    b = np.arange(P.shape[0])[:, None, None]
    t = (P[b, y0, x0], P[b, y0, x0 + 1], P[b, y0 + 1, x0], P[b, y0 + 1, x0 + 1])
    v = wts[0] * t[0]
    for k in (1, 2, 3):
        v = _fma(wts[k], t[k], v, dt)
    if want_mag:
        return v, sum(np.abs(wts[k] * t[k]) for k in range(4))
    return v


def linearize(a, b, flow, dtype=np.float64, want_mag=False):
    """coef [n][3][h][w] = (Ix, Iy, c) of luma planes a, b [n][h][w] at flow [n][2][h][w].
    want_mag: also the magnitude sums of the three (what their rounding errors scale with)."""
    dt = dtype
    a, b, flow = (np.asarray(t).astype(dt) for t in (a, b, flow))
    n, h, w = b.shape
    jp, jm = np.minimum(np.arange(w) + 1, w - 1), np.maximum(np.arange(w) - 1, 0)
    ip, im = np.minimum(np.arange(h) + 1, h - 1), np.maximum(np.arange(h) - 1, 0)
    bx = dt(0.5) * (b[:, :, jp] - b[:, :, jm])
    by = dt(0.5) * (b[:, ip] - b[:, im])
    y0, x0, wts = _taps(flow, dt)
    u, v = flow[:, 0], flow[:, 1]
    bw, mb = _sample(b, y0, x0, wts, dt, True)
    ix, _ = _sample(bx, y0, x0, wts, dt, True)
    iy, _ = _sample(by, y0, x0, wts, dt, True)
    with np.errstate(invalid="ignore", over="ignore"):
        c = _fma(iy, v, _fma(ix, u, a - bw, dt), dt)
    coef = np.stack([ix, iy, c], axis=1)
    if not want_mag:
        return coef
    # a gradient tap is 0.5 (B+ - B-): its magnitude 0.5 (|B+| + |B-|)
    mx = _sample(0.5 * (np.abs(b[:, :, jp]) + np.abs(b[:, :, jm])), y0, x0, wts, dt)
    my = _sample(0.5 * (np.abs(b[:, ip]) + np.abs(b[:, im])), y0, x0, wts, dt)
    with np.errstate(invalid="ignore", over="ignore"):
        mc = np.abs(a) + mb + mx * np.abs(u) + my * np.abs(v)
    return coef, np.stack([mx, my, mc], axis=1)


def _bar(p, dt, mag=False):
    q = np.pad(np.abs(p) if mag else p, ((0, 0), (1, 1), (1, 1)), mode="edge")
    N, S, W, E = q[:, :-2, 1:-1], q[:, 2:, 1:-1], q[:, 1:-1, :-2], q[:, 1:-1, 2:]
    NW, NE, SW, SE = q[:, :-2, :-2], q[:, :-2, 2:], q[:, 2:, :-2], q[:, 2:, 2:]
    e, d = (N + S) + (W + E), (NW + NE) + (SW + SE)
    c6 = np.float32(1.0) / np.float32(6.0) if dt == np.float32 else 1.0 / 6.0
    c12 = np.float32(1.0) / np.float32(12.0) if dt == np.float32 else 1.0 / 12.0
    return _fma(d, dt(c12), e * dt(c6), dt)


def jacobi(coef, uv, alpha=15.0, iters=40, dtype=np.float64, want_mag=False):
    """`iters` Jacobi iterations from uv.  want_mag (one iteration): also the magnitude sum
    of the update's terms."""
    dt = dtype
    coef, uv = np.asarray(coef).astype(dt), np.asarray(uv).astype(dt)
    ix, iy, c = coef[:, 0], coef[:, 1], coef[:, 2]
    a2 = dt(np.float32(alpha)) * dt(np.float32(alpha))
    ru, rv = dt(1) / _fma(ix, ix, a2, dt), dt(1) / _fma(iy, iy, a2, dt)
    u, v = uv[:, 0], uv[:, 1]
    for _ in range(iters):
        un = _fma(_fma(-iy, v, c, dt), ix, a2 * _bar(u, dt), dt) * ru
        vn = _fma(_fma(-ix, u, c, dt), iy, a2 * _bar(v, dt), dt) * rv
        mag = None
        if want_mag:
            mag = np.stack([((np.abs(c) + np.abs(iy * v)) * np.abs(ix) + a2 * _bar(u, dt, True)) * ru,
                            ((np.abs(c) + np.abs(ix * u)) * np.abs(iy) + a2 * _bar(v, dt, True)) * rv],
                           axis=1)
        u, v = un, vn
    out = np.stack([u, v], axis=1)
    return (out, mag) if want_mag else out


def estimate(A, B, dtype=np.float64, alpha=15.0, warps=5, iters=40, min_side=16, mean=MEAN,
             std=STD):
    """f [n][2][h][w] with A(i, j) ~ B(i + f[1], j + f[0]), A and B conditioned frames
    [n][3][h][w]."""
    dt = dtype
    ga, gb = [luma(A, mean, std, dt)], [luma(B, mean, std, dt)]
    levels = pyramid(ga[0].shape[1], ga[0].shape[2], min_side)
    for hl, wl in levels[1:]:
        ga.append(resize(ga[-1], hl, wl, dt))
        gb.append(resize(gb[-1], hl, wl, dt))
    uv = np.zeros((ga[0].shape[0], 2) + levels[-1], dt)
    for l in range(len(levels) - 1, -1, -1):
        for _ in range(warps):
            uv = jacobi(linearize(ga[l], gb[l], uv, dt), uv, alpha, iters, dt)
        if l:
            (hc, wc), (hf, wf) = levels[l], levels[l - 1]
            uv = resize(uv, hf, wf, dt)
            if dt == np.float32:
                sx, sy = np.float32(wf) / np.float32(wc), np.float32(hf) / np.float32(hc)
            else:
                sx, sy = wf / wc, hf / hc
            uv = np.stack([uv[:, 0] * dt(sx), uv[:, 1] * dt(sy)], axis=1)
    return uv


def estimate_pair(prev, cur, dtype=np.float64, **kw):
    """(fwd, bwd) of two frames: fwd = estimate(prev, cur), bwd = estimate(cur, prev), run as
    one batch of two."""
    f = estimate(np.concatenate([prev, cur]), np.concatenate([cur, prev]), dtype, **kw)
    return f[:1], f[1:]


# ------------------------------------------------------------------------ the test clips
def texture(h, w, seed, octaves=(8, 16, 32)):
    """[h][w] fp64 in 0..255: a sum of uniform noise at the octaves, cubic-resized."""
    rng = np.random.default_rng(seed)
    t = np.zeros((h, w))
    for o in octaves:
        t += scale_ref.resize(rng.uniform(0, 1, (-(-h // o) + 1, -(-w // o) + 1)), h, w, "cubic")
    t -= t.min()
    return t * (255.0 / t.max())


def condition(grey):
    """A 0..255 plane [h][w] as a conditioned grey frame [1][3][h][w] fp32."""
    g = np.asarray(grey, np.float64)[None, None] / 255.0
    return ((g - MEAN.astype(np.float64).reshape(1, 3, 1, 1)) /
            STD.astype(np.float64).reshape(1, 3, 1, 1)).astype(np.float32)


def smooth_field(h, w):
    """flow_ref.recipe's smooth field s(i, j) [1][2][h][w] as (dx, dy), without its rectangle
    and noise."""
    i = np.arange(h, dtype=np.float64)[:, None]
    j = np.arange(w, dtype=np.float64)[None, :]
    return np.stack([np.broadcast_to(2.5 * np.sin(np.pi * i / h + 0.3) + 1.0, (h, w)),
                     np.broadcast_to(2.0 * np.cos(np.pi * j / w + 0.7) - 0.5, (h, w))])[None]


@functools.lru_cache(maxsize=None)
def clip(kind, h, w, seed=8):
    """(A, B, f): conditioned frames [1][3][h][w] fp32 and the true flow [1][2][h][w] fp64 with
    A(p) = B(p + f) exactly under bilinear sampling: A is a padded canvas sampled at p + f,
    B the canvas at p.  kind: "translation" (dx, dy) = (5.25, -3.5) or "smooth"."""
    f = smooth_field(h, w) if kind == "smooth" else \
        np.broadcast_to(np.array([5.25, -3.5]).reshape(1, 2, 1, 1), (1, 2, h, w)).copy()
    pad = int(np.ceil(np.abs(f).max())) + 1
    canvas = texture(h + 2 * pad, w + 2 * pad, seed)[None, None]
    fp = np.pad(f, ((0, 0), (0, 0), (pad, pad), (pad, pad)), mode="edge")
    a, valid = flow_ref.warp(canvas, fp, coord_dtype=np.float64)
    assert valid[:, pad:-pad, pad:-pad].all()
    crop = lambda t: t[0, 0, pad:-pad, pad:-pad]
    return condition(crop(a)), condition(crop(canvas)), f


def interior(f, h, w):
    m = int(np.ceil(np.abs(f).max())) + 4
    return (slice(None), slice(m, h - m), slice(m, w - m))


def epe(est, true):
    """End-point error [n][h][w]."""
    d = np.asarray(est, np.float64) - true
    return np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2)


@functools.lru_cache(maxsize=None)
def occlusion_clip(dr, dc, seed=9):
    """(prev, cur, rect): 96 x 128 conditioned frames; a 32 x 40 rectangle of octave-(4, 8)
    texture over the octave-(8, 16, 32) background, at rows 30.., cols 40.. in prev and moved
    by (dr, dc) in cur.  rect = (r0, c0) of the rectangle in prev."""
    h, w, rh, rw, r0, c0 = 96, 128, 32, 40, 30, 40
    bg = texture(h, w, seed)
    fg = texture(rh, rw, seed + 1, (4, 8))
    prev, cur = bg.copy(), bg.copy()
    prev[r0:r0 + rh, c0:c0 + rw] = fg
    cur[r0 + dr:r0 + dr + rh, c0 + dc:c0 + dc + rw] = fg
    return condition(prev), condition(cur), (r0, c0, rh, rw)
