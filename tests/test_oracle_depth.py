"""The oracle's depth handling, pinned on the CPU.

The GPU depth tests (tests/test_gpu_depth.py) compare the kernels with one depth-D oracle
call, so the oracle's own walk over the depth axis is checked first: a depth-D
``cell_*`` / ``node_*`` call must equal, bit for bit, D depth-1 calls on the slices
``u[c:c+1]`` and ``F[:, c:c+1]`` -- the value of a component depends on nothing but that
component's array and column.  The same through the compiled reference Fortran
(``oracle/_ref``) where it is built.
"""
import numpy as np
import pytest

from oracle import oracle as ora
from oracle import ref
from test_gpu_parity import make_case  # noqa: E402

KERNELS = ["IB_4", "PIECEWISE_CUBIC"]
DEPTHS = [3, 4, 5, 9]


@pytest.fixture(scope="module", params=["oracle", "ref_O0"])
def backend(request):
    if request.param == "oracle":
        ora.lib()
        return None
    if not ref.available():
        pytest.skip("oracle/_ref/libleref_{O0,O2}.so not built (no reference tree or no flang at build time)")
    return ref.backend("O0")


def _arrays(geom, centering, depth, rng):
    shape = geom.array_shape(centering, 0, depth)
    return rng.uniform(-1, 1, shape)


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("centering", ["cell", "node"])
@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("kernel", KERNELS)
def test_depth_interp_equals_slices(backend, kernel, ndim, centering, depth):
    geom, X, idx, xs, _ = make_case(kernel, ndim, centering, seed=100 * depth + ndim)
    rng = np.random.default_rng(depth)
    f = ora.cell_interp if centering == "cell" else ora.node_interp
    head = (kernel, list(geom.dx), list(geom.x_lower), list(geom.ilower), list(geom.iupper), list(geom.gcw))
    u = _arrays(geom, centering, depth, rng)
    M = X.shape[0]
    Q = np.full((M, depth), 7.0)
    f(*head, u, idx, xs, X, Q, depth, backend=backend)
    listed = np.zeros(M, bool)
    listed[idx] = True
    assert (Q[~listed] == 7.0).all(), "unlisted markers must be untouched"
    assert np.abs(Q[listed]).max() > 0.1
    for c in range(depth):
        Qc = np.full((M, 1), 7.0)
        f(*head, u[c:c + 1].copy(), idx, xs, X, Qc, 1, backend=backend)
        assert np.array_equal(Q[:, c], Qc[:, 0]), f"component {c} of {depth}"
    # components are told apart: no two columns alike
    assert len({Q[listed][:, c].tobytes() for c in range(depth)}) == depth


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("centering", ["cell", "node"])
@pytest.mark.parametrize("ndim", [2, 3])
@pytest.mark.parametrize("kernel", KERNELS)
def test_depth_spread_equals_slices(backend, kernel, ndim, centering, depth):
    geom, X, idx, xs, _ = make_case(kernel, ndim, centering, seed=100 * depth + ndim + 50)
    rng = np.random.default_rng(depth + 20)
    f = ora.cell_spread if centering == "cell" else ora.node_spread
    head = (kernel, list(geom.dx), list(geom.x_lower), list(geom.ilower), list(geom.iupper), list(geom.gcw))
    u0 = _arrays(geom, centering, depth, rng)
    M = X.shape[0]
    F = rng.uniform(-1, 1, (M, depth))
    u = u0.copy()
    f(*head, u, idx, xs, X, F, depth, backend=backend)
    assert not np.array_equal(u, u0)
    for c in range(depth):
        uc = u0[c:c + 1].copy()
        f(*head, uc, idx, xs, X, F[:, c:c + 1].copy(), 1, backend=backend)
        assert np.array_equal(u[c], uc[0]), f"component {c} of {depth}"
        assert not np.array_equal(uc[0], u0[c])
