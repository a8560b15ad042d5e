"""GPU: the z-slab migration kernels against their numpy restatement, bit for bit.

k_slab_update, k_slab_partition, k_mig_pack and k_mig_unpack (le_aux.hip) were reached only
through the multi-process test of one uniform configuration, compared with torch's remainder.
Here they run in one process against tests/slab_ref.py on the positions where the wrap and
the owner can go wrong -- the box's ends and their neighbours in the doubles, -0.0, a
subnormal, every slab face -- for row counts around the 64-lane wave and the 256-row block,
every rank count from 1 to 8, both update schemes, device counts from 0 to the capacity and
buffer capacities that are exactly met.  Everything is exact: positions bit for bit, orders
and counts entry for entry.  Each overflow raises the device flag 8 at ctx.synchronize().
"""
import numpy as np
import pytest

import slab_ref as sr

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LS = [(1.0, 1.0, 1.0), (2.0, 0.75, 1.5)]
MS = [1, 63, 64, 65, 255, 256, 257, 1000, 70001]
SENT = -7.5e77


@pytest.fixture(scope="module")
def le():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ibamr_amd import le as _le
    return _le


@pytest.fixture(scope="module")
def ctx(le):
    return le.Context(0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits_equal(t, a):
    """A device float64 tensor and a numpy array, bit for bit."""
    h = np.ascontiguousarray(t.cpu().numpy())
    a = np.ascontiguousarray(a, dtype=np.float64)
    return h.shape == a.shape and np.array_equal(h.view(np.int64), a.view(np.int64))


def ranks_of(P):
    return range(P) if P <= 4 else (0, 3, P - 1)


def i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("scheme", ["euler", "trapezoidal"])
@pytest.mark.parametrize("P", [1, 2, 3, 4, 8])
def test_update_partition(le, ctx, P, scheme):
    """X_new, order and counts are the restatement's for every box, plane count, rank and row
    count; X_new lies in [0, L); with one rank the order is the identity."""
    for L in LS:
        for Nz in (48, 64):
            if Nz % P:
                continue
            for M in MS:
                X, U0, U1, dt = sr.edge_rows(L, Nz, P, M, seed=1000 * P + M)
                Xd, U0d, U1d = dev(X), dev(U0), dev(U1)
                for rank in ranks_of(P):
                    what = f"L={L} Nz={Nz} P={P} rank={rank} M={M} {scheme}"
                    Xn, order, counts = le.slab_update_partition(ctx, scheme, dt, Xd, U0d, L, Nz, P, rank,
                                                                 U1=U1d if scheme == "trapezoidal" else None)
                    rX, rorder, rcounts, _ = sr.update_partition(scheme, dt, X, U0, L, Nz, P, rank, U1=U1)
                    assert bits_equal(Xn, rX), f"{what}: X_new"
                    assert np.array_equal(counts.cpu().numpy(), rcounts), f"{what}: counts {counts.tolist()}"
                    assert np.array_equal(order.cpu().numpy(), rorder), f"{what}: order"
                    assert bool(((Xn >= 0.0) & (Xn < dev(np.array(L)))).all()), f"{what}: X_new outside [0, L)"
                    if P == 1:
                        assert torch.equal(order, torch.arange(M, dtype=torch.int32, device=DEV))
    ctx.synchronize()


@pytest.mark.parametrize("scheme", ["euler", "trapezoidal"])
@pytest.mark.parametrize("P,rank", [(4, 1), (2, 0), (1, 0)])
def test_update_partition_count(le, ctx, P, rank, scheme):
    """The first n_dev rows of capacity-sized arrays whose padding is NaN: the counts sum to
    n_dev, order[:n_dev] and X_new[:n_dev] are the restatement's on those rows."""
    L, Nz = LS[1], 48
    for C in (257, 1000):
        X, U0, U1, dt = sr.edge_rows(L, Nz, P, C, seed=77 + C)
        for n in (0, 1, 255, 256, C):
            what = f"P={P} rank={rank} C={C} n_dev={n} {scheme}"
            pad = [a.copy() for a in (X, U0, U1)]
            for a in pad:
                a[n:] = np.nan
            Xd, U0d, U1d = (dev(a) for a in pad)
            Xn, order, counts = le.slab_update_partition_count(ctx, scheme, dt, Xd, U0d, L, Nz, P, rank, i32([n]),
                                                               U1=U1d if scheme == "trapezoidal" else None)
            rX, rorder, rcounts, _ = sr.update_partition(scheme, dt, X, U0, L, Nz, P, rank, U1=U1, n=n)
            c = counts.cpu().numpy()
            assert c.sum() == n and np.array_equal(c, rcounts), f"{what}: counts {c}"
            assert np.array_equal(order[:n].cpu().numpy(), rorder), f"{what}: order"
            assert bits_equal(Xn[:n], rX), f"{what}: X_new"
            assert not torch.isnan(Xn[:n]).any()
    ctx.synchronize()


def partitioned_rows(le, ctx, P, rank, M, D, seed, far=False, capacity=None):
    """Rows of depth D (X_new, then random columns) partitioned on the device and in numpy.
    Without `far` the rows further than a neighbour are left out (the pack needs none)."""
    L, Nz = LS[1], 48
    X, U0, U1, dt = sr.edge_rows(L, Nz, P, M, seed=seed)
    if not far:
        keep = sr.update_partition("euler", dt, X, U0, L, Nz, P, rank)[3] != 3
        X, U0 = X[keep], U0[keep]
    n = X.shape[0]
    C = n if capacity is None else capacity
    pad = np.full((C - n, 3), np.nan)
    Xn, order, counts = le.slab_update_partition_count(ctx, "euler", dt, dev(np.concatenate([X, pad])),
                                                       dev(np.concatenate([U0, pad])), L, Nz, P, rank, i32([n]))
    rX, rorder, rcounts, _ = sr.update_partition("euler", dt, X, U0, L, Nz, P, rank)
    rng = np.random.default_rng(seed + 1)
    rows = rng.standard_normal((C, D))
    k = min(D, 3)
    rows[:n, :k] = rX[:, :k]
    assert np.array_equal(counts.cpu().numpy(), rcounts) and np.array_equal(order[:n].cpu().numpy(), rorder)
    return rows, dev(rows), order, counts, rorder, rcounts


@pytest.mark.parametrize("D", [1, 3, 7])
def test_pack(le, ctx, D):
    """The leavers in partition order in the first rows of each send buffer, the rest of the
    buffers untouched; a send_cap of exactly the larger count raises nothing."""
    for P, rank in ((4, 1), (2, 1), (8, 0), (3, 2)):
        for M in (65, 257, 1000, 70001):
            rows, rows_d, order, counts, rorder, rcounts = partitioned_rows(le, ctx, P, rank, M, D, seed=31 * P + M)
            n_down, n_up = int(rcounts[1]), int(rcounts[2])
            assert rcounts[3] == 0 and n_down > 0 and (n_up > 0 or P == 2)
            rdown, rup = sr.pack(rows, rorder, rcounts)
            for cap in (max(n_down, n_up), max(n_down, n_up) + 5):
                sd = torch.full((cap, D), SENT, dtype=torch.float64, device=DEV)
                su = torch.full_like(sd, SENT)
                le.slab_migrate_pack(ctx, rows_d, order, counts, sd, su)
                ctx.synchronize()  # an exactly met capacity raises nothing
                what = f"P={P} rank={rank} M={M} D={D} cap={cap}"
                assert bits_equal(sd[:n_down], rdown) and bits_equal(su[:n_up], rup), f"{what}: packed rows"
                assert bool((sd[n_down:] == SENT).all()) and bool((su[n_up:] == SENT).all()), f"{what}: rows past n"


@pytest.mark.parametrize("D", [1, 3, 7])
def test_unpack(le, ctx, D):
    """out = the stayers in partition order, the rows from below, the rows from above; the
    rows past n_out untouched; an out_cap of exactly n_out raises nothing."""
    rng = np.random.default_rng(5)
    for P, rank in ((4, 1), (2, 0), (8, 7)):
        for M in (65, 257, 1000, 70001):
            rows, rows_d, order, counts, rorder, rcounts = partitioned_rows(le, ctx, P, rank, M, D, seed=17 * P + M,
                                                                           capacity=M + 40)
            send_cap = 37
            for rd, ru in ((37, 0), (0, 37), (11, 29), (0, 0)):
                fd, fu = rng.standard_normal((send_cap, D)), rng.standard_normal((send_cap, D))
                want = sr.unpack(rows, rorder, rcounts, fd[:rd], fu[:ru])
                n_out = want.shape[0]
                for out_cap in (n_out, n_out + 9):
                    out = torch.full((out_cap, D), SENT, dtype=torch.float64, device=DEV)
                    n_dev = i32([-1])
                    le.slab_migrate_unpack(ctx, rows_d, order, counts, i32([rd, ru]), dev(fd), dev(fu), out, n_dev)
                    ctx.synchronize()  # an exactly met capacity raises nothing
                    what = f"P={P} rank={rank} M={M} D={D} from below {rd}, above {ru}, out_cap={out_cap}"
                    assert int(n_dev.item()) == n_out == int(rcounts[0]) + rd + ru, what
                    assert bits_equal(out[:n_out], want), f"{what}: unpacked rows"
                    assert bool((out[n_out:] == SENT).all()), f"{what}: rows past n_out"


@pytest.mark.parametrize("which", ["send_cap one short", "a row further than a neighbour", "recv_counts above send_cap",
                                   "arrivals beyond out_cap"])
def test_overflow_raises_flag_8(le, which):
    """Never a silent drop: each overflow sets the device flag 8, raised at synchronize().  A
    context of its own each, used for nothing afterwards."""
    ctx = le.Context(0)
    D = 3
    far = which == "a row further than a neighbour"
    rows, rows_d, order, counts, rorder, rcounts = partitioned_rows(le, ctx, 4, 1, 1000, D, seed=3, far=far)
    n_stay, n_down, n_up = (int(v) for v in rcounts[:3])
    ctx.synchronize()
    cap = max(n_down, n_up)
    n_dev = i32([-1])
    if which == "send_cap one short":
        cap -= 1
    if which in ("send_cap one short", "a row further than a neighbour"):
        assert (rcounts[3] > 0) == far
        sd = torch.full((cap, D), SENT, dtype=torch.float64, device=DEV)
        le.slab_migrate_pack(ctx, rows_d, order, counts, sd, torch.full_like(sd, SENT))
    else:
        send_cap = 20
        fd = torch.zeros((send_cap, D), dtype=torch.float64, device=DEV)
        over = which == "recv_counts above send_cap"
        rc = i32([send_cap + 1, 0] if over else [send_cap, send_cap])
        out_cap = n_stay + 2 * send_cap + (0 if over else -1)
        out = torch.full((out_cap, D), SENT, dtype=torch.float64, device=DEV)
        le.slab_migrate_unpack(ctx, rows_d, order, counts, rc, fd, fd.clone(), out, n_dev)
    with pytest.raises(RuntimeError, match="flag 8"):
        ctx.synchronize()
    if which == "arrivals beyond out_cap":
        assert int(n_dev.item()) == out_cap, "n_out is clamped to out_cap"
        assert bits_equal(out[:n_stay], rows[rorder[:n_stay]])


@pytest.mark.parametrize("P", [2, 3, 4, 8])
def test_step_in_one_process(le, ctx, P):
    """A P-rank step in one process: partition_count and pack per rank, the buffers routed as
    the neighbour exchange routes them (from below: the lower neighbour's send_up; from above:
    the upper neighbour's send_down), unpack per rank.  Every rank's rows and their order are
    the restatement's, the ids are a permutation, every row is on the owner of its wrapped cell."""
    L, Nz, M, D = LS[1], 48, 5003, 7
    C, send_cap = M + 1500, 800
    res, ref = [], []
    for r in range(P):
        X, U0, dt, F, ids = sr.step_rows(L, Nz, P, r, M, seed=200)
        pad = lambda a: dev(np.concatenate([a, np.full((C - M,) + a.shape[1:], np.nan)]))  # noqa: E731
        Xn, order, counts = le.slab_update_partition_count(ctx, "euler", dt, pad(X), pad(U0), L, Nz, P, r, i32([M]))
        data = torch.cat([Xn, pad(F), pad(ids[:, None])], dim=1).contiguous()
        sd = torch.full((send_cap, D), SENT, dtype=torch.float64, device=DEV)
        su = torch.full_like(sd, SENT)
        le.slab_migrate_pack(ctx, data, order, counts, sd, su)
        res.append((data, order, counts, sd, su))
        rX, rorder, rcounts, _ = sr.update_partition("euler", dt, X, U0, L, Nz, P, r)
        rrows = np.concatenate([rX, F, ids[:, None]], axis=1)
        ref.append((rrows, rorder, rcounts) + sr.pack(rrows, rorder, rcounts))
        assert 0.05 * M < rcounts[1] + rcounts[2] < 0.15 * M and rcounts[3] == 0
    ctx.synchronize()
    all_ids = []
    for r in range(P):
        dn, up = (r - 1) % P, (r + 1) % P
        data, order, counts = res[r][:3]
        rc = torch.stack([res[dn][2][2], res[up][2][1]])  # the lower neighbour's ups, the upper one's downs
        out = torch.full((C, D), SENT, dtype=torch.float64, device=DEV)
        n_dev = i32([-1])
        le.slab_migrate_unpack(ctx, data, order, counts, rc, res[dn][4], res[up][3], out, n_dev)
        ctx.synchronize()
        want = sr.unpack(ref[r][0], ref[r][1], ref[r][2], ref[dn][4], ref[up][3])
        n = int(n_dev.item())
        assert n == want.shape[0], f"rank {r}: {n} rows"
        assert bits_equal(out[:n], want), f"rank {r}: rows or their order"
        assert bool((out[n:] == SENT).all())
        o = out[:n].cpu().numpy()
        assert (sr.owner(o[:, 2], L[2], Nz, P) == r).all(), f"rank {r}: a row not on the owner of its cell"
        assert ((o[:, :3] >= 0.0) & (o[:, :3] < np.array(L))).all()
        all_ids.append(o[:, 6])
    assert np.array_equal(np.sort(np.concatenate(all_ids)), np.arange(P * M, dtype=np.float64)), "ids: a permutation"
