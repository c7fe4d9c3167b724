"""The Gram finalize's summation order over long chains of partials (gram.hip,
gram_finalize_body_g).  A split-lane of the finalize that owns more than one round of
partials issues several rounds of loads before it waits; every accumulator must still take
the same addends in the same order, so G is bit for bit what the documented order gives:

    split-lane kl (of KL = 32 / fin_groups(nsplit)) takes the partials k = kl (mod KL);
    they go round-robin into four accumulators while four more are left (k + 3 KL <
    nsplit), the remainder into the first; t = (s0 + s1) + (s2 + s3); the KL lane sums are
    added in lane order from 0; G = sum * scale.

The emulation below does exactly these float32 adds and the one multiply, so equality is
exact.  Both finalize forms are held to it: the immediate one of stx_style_loss (parts) and
the batched stx_gram_finalize_batch.  nsplit: one round, the remainder loop, several full
rounds, a ragged count, and conv1_2's 1024 at 512^2; c = 128 with 16 and 8 partials covers
the two- and four-sub-tile blocks, whose chains are a single partial.  A launch takes the
deep loop only when one of its jobs has a chain of four rounds, so the last test puts short,
two-round and long jobs into one batched launch: every job through the deep kernel."""
import numpy as np
import pytest
import torch

from styletransfer_amd import _native as N
from styletransfer_amd import ops

pytestmark = pytest.mark.gpu

HW = 96  # any pixel count: only the scale 1 / (c hw) and the workspace size depend on it


def fin_groups(nsplit):  # gram.hip
    return 4 if nsplit <= 8 else 2 if nsplit <= 16 else 1


def tile_sum(parts, kl_count):
    """parts [nsplit][4096] float32 -> the finalize's sum per tile element, float32."""
    nsplit = parts.shape[0]
    lanes = []
    for kl in range(kl_count):
        s = [np.zeros(parts.shape[1], np.float32) for _ in range(4)]
        ks = list(range(kl, nsplit, kl_count))
        full = len(ks) // 4 * 4
        for j, k in enumerate(ks[:full]):
            s[j % 4] = s[j % 4] + parts[k]
        for k in ks[full:]:
            s[0] = s[0] + parts[k]
        lanes.append((s[0] + s[1]) + (s[2] + s[3]))
    tot = np.zeros(parts.shape[1], np.float32)
    for t in lanes:
        tot = tot + t
    return tot


def emulate(parts, c, nsplit):
    """parts [U][nsplit][64][64] (U upper-triangle tiles, row-major) -> G [c][c]."""
    nt = c // 64
    scale = np.float32(1.0 / (float(c) * HW))
    g = np.zeros((c, c), np.float32)
    u = 0
    for i in range(nt):
        for j in range(i, nt):
            t = (tile_sum(parts[u].reshape(nsplit, 4096), 32 // fin_groups(nsplit)) * scale)
            t = t.reshape(64, 64)
            g[64 * i:64 * i + 64, 64 * j:64 * j + 64] = t
            if i != j:
                g[64 * j:64 * j + 64, 64 * i:64 * i + 64] = t.T
            u += 1
    return g


def test_emulation_is_a_sum():
    """The emulation against the fp64 sum (no GPU work): it adds every partial once."""
    rng = np.random.default_rng(5)
    for nsplit in (1, 31, 129, 515):
        p = rng.standard_normal((1, nsplit, 64, 64)).astype(np.float32)
        want = p[0].astype(np.float64).sum(0) / (64.0 * HW)
        got = emulate(p, 64, nsplit)
        assert np.abs(got - want).max() <= 1e-6 * max(1.0, np.abs(want).max()) * np.sqrt(nsplit)


CASES = [(64, 1), (64, 31), (64, 128), (64, 129), (64, 515), (64, 1024), (128, 16), (128, 8)]
_cases = {}


def case(dev, c, nsplit):
    """(partials on the device, the emulated G): computed once per case."""
    if (c, nsplit) not in _cases:
        U = 3 if c == 128 else 1
        rng = np.random.default_rng(100 + nsplit)
        parts = rng.standard_normal((U, nsplit, 64, 64)).astype(np.float32)
        _cases[c, nsplit] = (torch.from_numpy(parts).to(dev).reshape(-1),
                             emulate(parts, c, nsplit))
    return _cases[c, nsplit]


@pytest.mark.parametrize("c,nsplit", CASES)
def test_finalize_order(dev, c, nsplit):
    pd, want = case(dev, c, nsplit)
    target = torch.zeros(c, c, device=dev)
    got = []
    for batched in (False, True):
        ws = torch.empty(N.lib().stx_gram_ws(1, c, HW), device=dev, dtype=torch.uint8)
        g = torch.full((1, c, c), float("nan"), device=dev)
        fin = ops.FinalizeBatch() if batched else None
        _, coef = ops._style_loss(1, c, HW, target, dev, 1.0, 0.0, None, ws, fin, parts=pd,
                                  nparts=nsplit, g_out=g)  # (coef: alive until the flush)
        if fin is not None:
            assert len(fin.jobs) == 1
            fin.flush()
        torch.cuda.synchronize()
        got.append(g[0].cpu().numpy())
    assert np.array_equal(got[0], want), np.abs(got[0] - want).max()
    assert np.array_equal(got[1], want), np.abs(got[1] - want).max()


def test_finalize_order_mixed_batch(dev):
    """Jobs of one round, two rounds (256), a ragged long chain, the longest and the
    sub-tiled short ones in ONE batched launch."""
    mixed = [(64, 129), (64, 256), (64, 515), (128, 16), (64, 1024), (64, 31), (128, 8)]
    fin, runs = ops.FinalizeBatch(), []
    for c, nsplit in mixed:
        pd, want = case(dev, c, nsplit)
        ws = torch.empty(N.lib().stx_gram_ws(1, c, HW), device=dev, dtype=torch.uint8)
        g = torch.full((1, c, c), float("nan"), device=dev)
        target = torch.zeros(c, c, device=dev)
        _, coef = ops._style_loss(1, c, HW, target, dev, 1.0, 0.0, None, ws, fin, parts=pd,
                                  nparts=nsplit, g_out=g)
        runs.append((g, want, ws, target, coef))  # (all alive until the flush)
    assert len(fin.jobs) == len(mixed)
    fin.flush()
    torch.cuda.synchronize()
    for (c, nsplit), (g, want, *_) in zip(mixed, runs):
        assert np.array_equal(g[0].cpu().numpy(), want), (c, nsplit)
