"""GPU: the re-key pass of the re-binning (k_rekey) at the sizes where its row loop ends.

A workgroup of k_rekey takes ROWS rows of 256 consecutive sorted entries, every load of
a row issued before the first key is computed; rows past the list's end load its last
entry again and store nothing.  Each case re-bins a list and compares it with a fresh
binning of the same list at the same positions, as test_gpu_rebin.py does: the canonical
order must be equal, and a side IB_4 interp and spread through the two must be bitwise
equal -- that covers the keys, the bucket starts, the sorted positions and the sweep item
table, none of which the library hands out.  The list lengths are the edges of a wave
(64), of a row (256) and of a workgroup (ROWS * 256), and a length with two full
workgroups and a partial wave; the patch has several columns in x and y.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

ROWS, BLOCK = 4, 256   # RK_ROWS, BLOCK (le_sweep.hip)
N = (64, 32, 32)
LENGTHS = [1, 63, 64, 65, 255, 256, 257, ROWS * BLOCK - 1, ROWS * BLOCK, ROWS * BLOCK + 1, 2 * ROWS * BLOCK + 33]
PATTERNS = ["none", "first", "last", "all"]


@pytest.fixture(scope="module")
def le():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ibamr_amd import le as _le
    return _le


@pytest.fixture(scope="module")
def env(le):
    """The patch, a context and the Eulerian field every case interpolates (unchanged)."""
    geom = le.Geometry.periodic_unit(list(N), 3)
    rng = np.random.default_rng(21)
    u = geom.alloc("side")
    for a in u:
        a.copy_(torch.from_numpy(rng.uniform(-1, 1, tuple(a.shape))))
    return geom, le.Context(0), u


def _positions(rng, M, lo=0.1, hi=0.4):
    """M markers at cell + [lo, hi) in every direction: a move of less than 0.05 cells
    crosses neither a cell face nor a cell centre, so no key and no shifted anchor changes."""
    c = np.stack([rng.integers(0, N[d], M) for d in range(3)], axis=1)
    return (c + rng.uniform(lo, hi, (M, 3))) / np.array(N)


def _run(le, ctx, m, geom, u, X, F, kernel="IB_4"):
    U = torch.zeros((F.shape[0], 3), dtype=torch.float64, device="cuda")
    le.interp(ctx, m, kernel, "side", geom, u, U, X)
    f = geom.alloc("side")
    le.spread(ctx, m, kernel, "side", geom, f, F, X)
    ctx.synchronize()
    return U, f


def _same(le, ctx, geom, u, m_re, m_fr, X, F):
    assert torch.equal(m_re.order(), m_fr.order())
    U1, f1 = _run(le, ctx, m_re, geom, u, X, F)
    U2, f2 = _run(le, ctx, m_fr, geom, u, X, F)
    assert torch.equal(U1, U2)
    for a, b in zip(f1, f2):
        assert torch.equal(a, b)


def _moved(X, order, pattern):
    """X after a sub-cell move of every marker (the sorted positions change, no key does),
    and the pattern's movers one cell further in z."""
    X2 = X + 0.03 / max(N)
    dz = 1.0 / N[2]
    if pattern == "first":
        i = int(order[0])
        X2[i, 2] = (X2[i, 2] + dz) % 1.0
    elif pattern == "last":
        i = int(order[-1])
        X2[i, 2] = (X2[i, 2] + dz) % 1.0
    elif pattern == "all":
        X2[:, 2] = torch.remainder(X2[:, 2] + dz, 1.0)
    return X2


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("M", LENGTHS)
def test_rekey_rows_equal_fresh_bin(le, env, M, pattern):
    geom, ctx, u = env
    rng = np.random.default_rng(1000 + M)
    X = torch.from_numpy(_positions(rng, M)).cuda()
    F = torch.from_numpy(rng.standard_normal((M, 3))).cuda()
    m = le.Markers(ctx).bin(geom, "IB_4", X)
    X2 = _moved(X, m.order().cpu(), pattern)
    m.rebin(X2)
    _same(le, ctx, geom, u, m, le.Markers(ctx).bin(geom, "IB_4", X2), X2, F)
    m.rebin(X)   # and back: the counters and the bit words left by the first are clean
    _same(le, ctx, geom, u, m, le.Markers(ctx).bin(geom, "IB_4", X), X, F)


@pytest.mark.parametrize("n", [ROWS * BLOCK + 1, 2 * ROWS * BLOCK + 33])
def test_rekey_rows_index_list_with_shifts(le, env, n):
    """The index-list form (indices + Xshift): the first n entries of a periodic list."""
    geom, ctx, u = env
    rng = np.random.default_rng(2000 + n)
    M = 2000
    X = torch.from_numpy(rng.uniform(0.0, 1.0, (M, 3))).cuda()
    F = torch.from_numpy(rng.standard_normal((M, 3))).cuda()
    idx, xs = le.periodic_index_list(ctx, geom, X, 3)
    assert idx.numel() >= n
    idx, xs = idx[:n].contiguous(), xs.reshape(-1, 3)[:n].contiguous()
    m = le.Markers(ctx).bin(geom, "IB_4", X, idx, xs)
    h = torch.tensor([1.0 / v for v in N], dtype=torch.float64, device="cuda")
    X2 = X + 0.4 * h * (torch.rand_like(X) - 0.5)   # a fraction of the entries change bucket
    m.rebin(X2)
    assert m.count() == n
    _same(le, ctx, geom, u, m, le.Markers(ctx).bin(geom, "IB_4", X2, idx, xs), X2, F)
    m.rebin(X2)   # nothing moved
    _same(le, ctx, geom, u, m, le.Markers(ctx).bin(geom, "IB_4", X2, idx, xs), X2, F)


@pytest.mark.parametrize("cap,M", [(ROWS * BLOCK + 100, ROWS * BLOCK - 24), (2 * ROWS * BLOCK + 33, ROWS * BLOCK + 1)])
def test_rekey_rows_fixed_capacity(le, env, cap, M):
    """A fixed-capacity list (bin_count) whose count is below its capacity: the rows past
    the count exist, are read and keep the outside key."""
    geom, ctx, u = env
    rng = np.random.default_rng(3000 + cap)
    X = torch.zeros((cap, 3), dtype=torch.float64, device="cuda")
    X[:M] = torch.from_numpy(_positions(rng, M)).cuda()
    F = torch.from_numpy(rng.standard_normal((cap, 3))).cuda()
    cnt = lambda: torch.tensor([M], dtype=torch.int32, device="cuda")
    c0 = cnt()
    m = le.Markers(ctx).bin_count(geom, "IB_4", X, c0)
    X2 = X.clone()
    X2[:M] = _moved(X[:M], torch.arange(M), "none")
    X2[:M:3, 2] = torch.remainder(X2[:M:3, 2] + 1.0 / N[2], 1.0)   # every third a cell up in z
    m.rebin(X2)
    c1 = cnt()
    _same(le, ctx, geom, u, m, le.Markers(ctx).bin_count(geom, "IB_4", X2, c1), X2, F)


@pytest.mark.parametrize("M", [65, 2 * ROWS * BLOCK + 33])
def test_rekey_rows_subcell_move_flips_shifted_anchors(le, env, M):
    """A move within the cells that changes no key but every anchor in the frame shifted by
    -dz/2: the parity words of the last, partial wave (zbits) and their state (zst) must send
    the split candidate stream to be rebuilt, and an unchanged re-binning must keep it."""
    geom, ctx, u = env
    rng = np.random.default_rng(4000 + M)
    Xn = _positions(rng, M)
    k = rng.integers(1, N[2] - 1, M)
    Xn[:, 2] = (k - rng.uniform(0.15, 0.25, M)) / N[2]     # z / dz in k - [0.15, 0.25]
    X = torch.from_numpy(Xn).cuda()
    F = torch.from_numpy(rng.standard_normal((M, 3))).cuda()
    Fn = torch.from_numpy(rng.standard_normal((M, 1))).cuda()

    def node_same(mk, Xc):
        out = []
        for q in (mk, le.Markers(ctx).bin(geom, "IB_4", Xc)):
            f = geom.alloc("node", depth=1)
            le.spread(ctx, q, "IB_4", "node", geom, f, Fn, Xc)
            ctx.synchronize()
            out.append(f)
        for a, b in zip(*out):
            assert torch.equal(a, b)

    m = le.Markers(ctx).bin(geom, "IB_4", X)
    _same(le, ctx, geom, u, m, le.Markers(ctx).bin(geom, "IB_4", X), X, F)      # the split stream built
    m.rebin(X)                                                                   # nothing changed
    m.rebin(X)                                                                   # ... again (the parities compared)
    _same(le, ctx, geom, u, m, le.Markers(ctx).bin(geom, "IB_4", X), X, F)
    X2 = X.clone()
    X2[:, 2] += 0.35 / N[2]                                                      # z / dz in k + [0.1, 0.2]: the same cells
    m.rebin(X2)
    _same(le, ctx, geom, u, m, le.Markers(ctx).bin(geom, "IB_4", X2), X2, F)
    node_same(m, X2)
    m.rebin(X2)                                                                  # nothing changed: the stream stands
    _same(le, ctx, geom, u, m, le.Markers(ctx).bin(geom, "IB_4", X2), X2, F)
    X3 = X.clone()
    last = int(m.order()[-1])
    X3[last, 2] = X2[last, 2]                                                    # back, but for the last sorted entry
    m.rebin(X3)
    _same(le, ctx, geom, u, m, le.Markers(ctx).bin(geom, "IB_4", X3), X3, F)
    node_same(m, X3)
