"""Plain numpy fp64 restatement of the flow definitions (include/stx.h): the
yardstick of tests/test_flow_gpu.py, itself pinned by tests/test_flow_ref_host.py.

Images and flows are NCHW with h, w >= 2; a flow's channel 0 is the column displacement
dx, channel 1 the row displacement dy.  Pixel (i, j) samples at y = i + dy, x = j + dx.
Coordinates are formed in `coord_dtype` (fp32 by default, as the kernels form them: the
validity test is made on the fp32 coordinate as computed) and everything after that in
fp64."""
import numpy as np


def coords(flow, coord_dtype=np.float32):
    """(y, x) [n][h][w] in fp64, each rounded once to coord_dtype."""
    flow = np.asarray(flow)
    n, _, h, w = flow.shape
    f = flow.astype(coord_dtype)
    ii = np.arange(h, dtype=coord_dtype)[None, :, None]
    jj = np.arange(w, dtype=coord_dtype)[None, None, :]
    with np.errstate(invalid="ignore"):
        y = (ii + f[:, 1]).astype(np.float64)
        x = (jj + f[:, 0]).astype(np.float64)
    return y, x


def warp(a, flow, fill=None, coord_dtype=np.float32, want_mag=False):
    """(out [n][c][h][w] fp64, valid [n][h][w] bool): a sampled bilinearly at (y, x);
    an invalid pixel takes fill's value (0 without fill) and reads no tap.  All four taps
    enter the sum, also under a zero weight.  want_mag: also sum_k |w_k a_k|."""
    a = np.asarray(a, dtype=np.float64)
    n, c, h, w = a.shape
    y, x = coords(flow, coord_dtype)
    with np.errstate(invalid="ignore"):
        valid = (y >= 0) & (y <= h - 1) & (x >= 0) & (x <= w - 1)
    ys, xs = np.where(valid, y, 0.0), np.where(valid, x, 0.0)
    y0 = np.minimum(np.floor(ys), h - 2).astype(np.int64)
    x0 = np.minimum(np.floor(xs), w - 2).astype(np.int64)
    fy, fx = ys - y0, xs - x0
    b = np.arange(n)[:, None, None]
    out = np.zeros_like(a)
    mag = np.zeros_like(a)
    with np.errstate(invalid="ignore"):
        for k in range(c):
            p = a[:, k]
            terms = [(1 - fy) * (1 - fx) * p[b, y0, x0], (1 - fy) * fx * p[b, y0, x0 + 1],
                     fy * (1 - fx) * p[b, y0 + 1, x0], fy * fx * p[b, y0 + 1, x0 + 1]]
            out[:, k] = terms[0] + terms[1] + terms[2] + terms[3]
            mag[:, k] = sum(np.abs(t) for t in terms)
    other = np.zeros_like(a) if fill is None else np.asarray(fill, dtype=np.float64)
    out = np.where(valid[:, None], out, other)
    mag = np.where(valid[:, None], mag, 0.0)
    return (out, valid, mag) if want_mag else (out, valid)


def gradient(u):
    """(d/dcolumn, d/drow) of [n][h][w]: central difference halved in the interior,
    one-sided and unhalved in the first and last column / row."""
    gx, gy = np.empty_like(u), np.empty_like(u)
    with np.errstate(invalid="ignore"):
        gx[:, :, 1:-1] = (u[:, :, 2:] - u[:, :, :-2]) * 0.5
        gx[:, :, 0] = u[:, :, 1] - u[:, :, 0]
        gx[:, :, -1] = u[:, :, -1] - u[:, :, -2]
        gy[:, 1:-1] = (u[:, 2:] - u[:, :-2]) * 0.5
        gy[:, 0] = u[:, 1] - u[:, 0]
        gy[:, -1] = u[:, -1] - u[:, -2]
    return gx, gy


def consistency(fwd, bwd, coord_dtype=np.float32):
    """dict of [n][h][w] arrays: c (bool) = valid and not occluded and not boundary, the
    three tests, and each test's relative margin |lhs - rhs| / rhs (inf where the pixel is
    invalid for the occlusion test: it decides nothing there; NaN where an operand is)."""
    fwd = np.asarray(fwd, dtype=np.float64)
    bwd = np.asarray(bwd, dtype=np.float64)
    wt, valid = warp(fwd, bwd, coord_dtype=coord_dtype)
    u, v = bwd[:, 0], bwd[:, 1]
    with np.errstate(invalid="ignore"):
        m_b = u * u + v * v
        lo = (wt[:, 0] + u) ** 2 + (wt[:, 1] + v) ** 2
        ro = 0.01 * ((wt[:, 0] ** 2 + wt[:, 1] ** 2) + m_b) + 0.5
        occluded = valid & (lo > ro)
        ux, uy = gradient(u)
        vx, vy = gradient(v)
        lb = (ux * ux + uy * uy) + (vx * vx + vy * vy)
        rb = 0.01 * m_b + 0.002
        boundary = lb > rb
        margin_o = np.where(valid, np.abs(lo - ro) / ro, np.inf)
        margin_b = np.abs(lb - rb) / rb
    return dict(c=valid & ~occluded & ~boundary, valid=valid, occluded=occluded,
                boundary=boundary, margin_occluded=margin_o, margin_boundary=margin_b)


def masked_mse(x, ref, mask, weight):
    """(L, dL/dx, sum|terms| of L): L = weight / (n c h w) * sum over mask != 0 of
    (x - ref)^2; the mask [n][h][w] selects (nothing of an unselected pixel gets through)."""
    x = np.asarray(x, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    on = np.broadcast_to((np.asarray(mask) != 0)[:, None], x.shape)
    with np.errstate(invalid="ignore"):
        d = np.where(on, x - ref, 0.0)
    s = float(weight) / x.size
    return s * float((d * d).sum()), 2.0 * s * d, s * float((d * d).sum())


def temporal_error(y, y_prev, fwd, bwd):
    """sum c (y - W(y_prev, bwd))^2 / sum c: the masked temporal error of two stylised
    frames (per element of the selected pixels' three channels)."""
    om, _ = warp(y_prev, bwd)
    c = consistency(fwd, bwd)["c"]
    d = np.where(c[:, None], np.asarray(y, dtype=np.float64) - om, 0.0)
    return float((d * d).sum() / max(int(c.sum()), 1))


# ------------------------------------------------------------------ the mask tests' flows
def recipe(h, w, seed=7, n=1):
    """(fwd, bwd) fp32 [n][2][h][w]: a smooth field s(i, j) = (2.5 sin(pi i / h + 0.3) + 1,
    2 cos(pi j / w + 0.7) - 0.5) as (dx, dy), bwd = s and fwd = -s; the rectangle rows
    h/4..h/2, cols w/4..w/2 of bwd set to (dx, dy) = (5, -4), the same rectangle moved by
    (-4, +5) in (rows, cols) set in fwd to (-5, 4); uniform noise in +-0.01 on both, then
    rounded to multiples of 1/64 so that i + f is exact in fp32."""
    rng = np.random.default_rng(seed)
    i = np.arange(h, dtype=np.float64)[:, None]
    j = np.arange(w, dtype=np.float64)[None, :]
    s = np.stack([np.broadcast_to(2.5 * np.sin(np.pi * i / h + 0.3) + 1.0, (h, w)),
                  np.broadcast_to(2.0 * np.cos(np.pi * j / w + 0.7) - 0.5, (h, w))])
    bwd = np.repeat(s[None], n, axis=0).copy()
    fwd = -bwd
    r0, r1, c0, c1 = h // 4, h // 2, w // 4, w // 2
    bwd[:, 0, r0:r1, c0:c1], bwd[:, 1, r0:r1, c0:c1] = 5.0, -4.0
    q0, q1 = max(r0 - 4, 0), max(r1 - 4, 0)  # (a 5 x 7 image: the moved rectangle is cut)
    fwd[:, 0, q0:q1, c0 + 5:c1 + 5], fwd[:, 1, q0:q1, c0 + 5:c1 + 5] = -5.0, 4.0
    bwd += rng.uniform(-0.01, 0.01, bwd.shape)
    fwd += rng.uniform(-0.01, 0.01, fwd.shape)
    q = lambda f: (np.round(f * 64.0) / 64.0).astype(np.float32)
    return q(fwd), q(bwd)
