"""
Phase integration on the GPU (libumpa_integrate.so): b, d and the V-cycle bit for bit against the numpy restatement of
include/umpa_integrate.h (tests/integrate_expect.py), the tail kernel against the launched levels, the reductions against
extended precision, the solve against a dense least-squares solution, the gauge, fill, determinism, device tensors,
streams, batches, and phase_from_match.

REACHES names, per test, the kernels of libumpa_integrate.so it is there for (tests/test_integrate_cpu.py checks on the CPU
that every kernel symbol of the built library is claimed here, and that no claim is stale).
"""
import importlib

import numpy as np
import pytest

import integrate_expect as E

pytestmark = pytest.mark.gpu

_K = "integrate_%s_kernel"
REACHES = {
    "tests/test_hip_integrate.py::test_b_and_d_bit_for_bit": [_K % k for k in ("weights", "diag", "rhs", "coarsen")],
    "tests/test_hip_integrate.py::test_vcycle_bit_for_bit": [_K % k for k in ("tail",)],
    "tests/test_hip_integrate.py::test_tail_and_launched_levels_are_bit_identical":
        [_K % k for k in ("sweep0", "sweep", "restrict", "prolong", "tail")],
    "tests/test_hip_integrate.py::test_solve_against_the_dense_solution":
        [_K % k for k in ("apply_dot", "update", "residual", "dot", "direction", "gauge", "output", "scalar")],
    "tests/test_hip_integrate.py::test_jacobi_preconditioner_is_the_diagonal": [_K % "jacobi"],
}

BIT_SHAPES = E.SHAPES + E.SMALL
KINDS = ["ones", "holes"]
# 70 x 72 with its five coarser levels is the largest hierarchy of this aspect that fits the tail's LDS (3 * 6739 doubles
# of 20480), 70 x 73 (3 * 6871) the first that does not: there level 0 is launched and the tail starts at 35 x 37
TAIL_SHAPES = [(200, 333), (70, 72), (70, 73)]
_ids = lambda s: "%dx%d" % s                                          # noqa: E731


@pytest.fixture(scope="module")
def I():
    from umpa_amd import _lib
    if _lib.hip().device_count() < 1:
        pytest.fail("no HIP device: the GPU tests cannot run (there is no CPU fallback)")
    return importlib.import_module("umpa_amd.integrate")


def inputs(shape, kind):
    gx, gy, w, _ = E.case(E.case_name(shape, kind))
    return gx, gy, (w if kind == "holes" else None)


_solved = {}


def solved(I, shape, kind):
    """the default solve of a case on host arrays, made once"""
    key = (shape, kind)
    if key not in _solved:
        _solved[key] = I.integrate(*inputs(shape, kind))
    return _solved[key]


def check_residual(res, gx, gy, w, tol):
    """the reported residual against the 80-bit norm of b - L phi recomputed from the downloaded map"""
    w0 = E.weights0(gx, gy, w)
    b = E.rhs(w0, gx, gy)
    x = np.where(E.diag(w0) > 0, res.phi, 0.0)
    want, bound = E.true_residual(w0, b, x)
    print("   residual %.6e, extended %.6e, |difference| / bound = %.3f" % (res.residual, want, abs(res.residual - want) / bound))
    assert abs(res.residual - want) <= bound
    if res.status == I_CONVERGED:
        assert res.residual <= tol


I_CONVERGED = E.CONVERGED


# ----------------------------------------------------------------------------- 1. bit for bit against the restatement

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", BIT_SHAPES, ids=_ids)
def test_b_and_d_bit_for_bit(I, shape, kind):
    gx, gy, w = inputs(shape, kind)
    w0 = E.weights0(gx, gy, w)
    np.testing.assert_array_equal(I.rhs(gx, gy, w), E.rhs(w0, gx, gy))                     # solve with F_DEBUG
    np.testing.assert_array_equal(I.vcycle(np.zeros(shape), w, diagonal=True), E.diag(w0))  # vcycle with F_DEBUG
    if kind == "holes":                                               # without w: weight 1 where the gradients are finite
        w1 = E.weights0(gx, gy, None)
        np.testing.assert_array_equal(I.rhs(gx, gy, None), E.rhs(w1, gx, gy))
        assert np.isfinite(I.rhs(gx, gy, None)).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", BIT_SHAPES, ids=_ids)
def test_vcycle_bit_for_bit(I, shape, kind):
    gx, gy, w = inputs(shape, kind)
    r = np.random.default_rng(shape[0] * shape[1]).standard_normal(shape)
    want = E.vcycle(E.levels(E.weights0(gx, gy, w)), r)
    np.testing.assert_array_equal(I.vcycle(r, w), want)
    np.testing.assert_array_equal(I.vcycle(r, w, no_tail=True), want)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", TAIL_SHAPES, ids=_ids)
def test_tail_and_launched_levels_are_bit_identical(I, shape, kind):
    gx, gy, w = inputs(shape, kind)
    levels = E.levels(E.weights0(gx, gy, w))
    if shape == (200, 333):
        assert len(levels) >= 4                                       # F_NO_TAIL launches at least three levels above the coarsest
    r = np.random.default_rng(7).standard_normal(shape)
    a, b = I.vcycle(r, w), I.vcycle(r, w, no_tail=True)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, E.vcycle(levels, r))
    sa, sb = I.integrate(gx, gy, w), I.integrate(gx, gy, w, no_tail=True)
    np.testing.assert_array_equal(sa.phi, sb.phi)
    assert (sa.iterations, sa.residual, sa.status) == (sb.iterations, sb.residual, sb.status)


def test_jacobi_preconditioner_is_the_diagonal(I):
    gx, gy, w = inputs((33, 47), "holes")
    w0 = E.weights0(gx, gy, w)
    r = np.random.default_rng(8).standard_normal((33, 47))
    np.testing.assert_array_equal(I.vcycle(r, w, jacobi=True), E.jacobi0(E.diag(w0), r))
    res = I.integrate(gx, gy, w, jacobi=True, maxiter=3000)
    want = E.pcg(gx, gy, w, maxiter=3000, jacobi=True)
    print("jacobi: %d iterations (restated %d), V-cycle %d" % (res.iterations, want[1], solved(I, (33, 47), "holes").iterations))
    assert res.status == I.CONVERGED and abs(res.iterations - want[1]) <= max(2, want[1] // 50)
    assert res.iterations > 4 * solved(I, (33, 47), "holes").iterations


# ----------------------------------------------------------------------------- 2. reductions and the solve

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", E.SHAPES + E.SMALL, ids=_ids)
def test_reported_residual_against_extended_precision(I, shape, kind):
    gx, gy, w = inputs(shape, kind)
    res = solved(I, shape, kind)
    assert res.status == I.CONVERGED
    check_residual(res, gx, gy, w, 1e-10)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", E.SHAPES, ids=_ids)
def test_solve_against_the_dense_solution(I, shape, kind):
    """The GPU's dots sum in another order than the restatement's, so its iterates differ in the last bits while both
    stop on the same criterion: 4 x the deviation recorded for the restated solve, and its iteration count +- 2."""
    name = E.case_name(shape, kind)
    res = solved(I, shape, kind)
    rec = E.observed()[name]
    dev = E.deviation(res.phi, name)
    print("%s: %d iterations (recorded %d), deviation %.3e (recorded %.3e)" % (name, res.iterations, rec["iterations"], dev, rec["deviation"]))
    assert res.status == I.CONVERGED
    assert dev <= 4.0 * rec["deviation"]
    assert abs(res.iterations - rec["iterations"]) <= 2


# ----------------------------------------------------------------------------- 3. fill, gauge, b = 0, maxiter

def test_fill_gauge_zero_rhs_and_maxiter(I):
    shape = (37, 130)
    gx, gy, w = inputs(shape, "holes")
    d = E.diag(E.weights0(gx, gy, w))
    off = d == 0
    assert off.any()
    res = solved(I, shape, "holes")
    assert np.isnan(res.phi[off]).all() and np.isfinite(res.phi[~off]).all()
    filled = I.integrate(gx, gy, w, fill=-7.5)
    assert (filled.phi[off] == -7.5).all()
    np.testing.assert_array_equal(filled.phi[~off], res.phi[~off])
    # the gauge: the mean over the d > 0 pixels is zero within the rounding of the sum and of the subtraction
    n = int((~off).sum())
    mean = float(res.phi[~off].astype(np.longdouble).sum()) / n
    bound = (n + 2) * 2.0 ** -53 * np.abs(res.phi[~off]).sum() / n + 2.0 ** -53 * np.abs(res.phi[~off]).max()
    print("gauge: mean %.2e, bound %.2e" % (mean, bound))
    assert abs(mean) <= bound
    # b = 0
    zero = I.integrate(np.zeros(shape), np.zeros(shape), w)
    assert zero.iterations == 0 and zero.status == I.CONVERGED and zero.residual == 0.0
    assert (zero.phi[~off] == 0).all() and np.isnan(zero.phi[off]).all()
    # maxiter
    short = I.integrate(gx, gy, w, maxiter=3)
    assert short.status == I.MAXITER and short.iterations == 3 and np.isfinite(short.phi[~off]).all() and short.residual > 1e-10
    check_residual(short, gx, gy, w, 1e-10)
    none = I.integrate(gx, gy, w, maxiter=0)
    assert none.status == I.MAXITER and none.iterations == 0 and none.residual == 1.0 and (none.phi[~off] == 0).all()
    # an iteration count that is no multiple of the interval at which the host reads the flags, and one that is
    from umpa_amd import _lib
    for m in (_lib.INTEGRATE_CHECK_EVERY, _lib.INTEGRATE_CHECK_EVERY + 1):
        part = I.integrate(gx, gy, w, maxiter=m)
        want = E.pcg(gx, gy, w, maxiter=m)
        assert part.iterations == m == want[1] and part.status == I.MAXITER
        assert np.abs(part.phi[~off] - want[0][~off]).max() <= 1e-9 * np.abs(want[0][~off]).max()


def test_garbage_at_weight_zero_changes_nothing(I):
    shape = (33, 47)
    gx, gy, w = inputs(shape, "holes")
    res = solved(I, shape, "holes")
    gx2, gy2 = gx.copy(), gy.copy()
    gx2[w == 0], gy2[w == 0] = 1e30, -np.inf
    other = I.integrate(gx2, gy2, w)
    np.testing.assert_array_equal(res.phi, other.phi)
    assert (res.iterations, res.residual) == (other.iterations, other.residual)


# ----------------------------------------------------------------------------- 4. determinism, device tensors, streams, batches

def test_repeats_device_tensors_side_stream_and_batch_are_bit_identical(I):
    import torch
    shape = (37, 130)
    gx, gy, w = inputs(shape, "holes")
    res = solved(I, shape, "holes")
    again = I.integrate(gx, gy, w)
    np.testing.assert_array_equal(res.phi, again.phi)
    assert (res.iterations, res.residual, res.status) == (again.iterations, again.residual, again.status)
    r = np.nan_to_num(gx, nan=0.0)
    tg = [torch.from_numpy(a.copy()).cuda() for a in (gx, gy, w)]              # copies only: no torch kernel is launched
    tr = torch.from_numpy(r).cuda()
    dev = I.integrate(*tg)
    assert dev.phi.is_cuda and dev.phi.dtype == torch.float64
    np.testing.assert_array_equal(dev.phi.cpu().numpy(), res.phi)
    assert (dev.iterations, dev.residual, dev.status) == (res.iterations, res.residual, res.status)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = I.integrate(*tg)
        z_side = I.vcycle(tr, tg[2])
    side.synchronize()
    np.testing.assert_array_equal(on_side.phi.cpu().numpy(), res.phi)
    np.testing.assert_array_equal(z_side.cpu().numpy(), I.vcycle(r, w))
    with pytest.raises(ValueError, match="contiguous HIP tensors"):
        I.integrate(tg[0].t().contiguous().t(), tg[1], tg[2])
    with pytest.raises(ValueError, match="not mixed"):
        I.integrate(tg[0], gy, tg[2])
    # a batch of three maps equals three calls
    cases = [inputs(shape, "holes"), inputs(shape, "ones"), (gy.copy(), gx.copy(), w)]
    bg = [np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases]), np.stack([w, np.ones(shape), w])]
    batch = I.integrate(*bg)
    tbatch = I.integrate(*[torch.from_numpy(a).cuda() for a in bg])
    assert batch.phi.shape == (3,) + shape and batch.iterations.shape == (3,)
    for k in range(3):
        one = I.integrate(bg[0][k], bg[1][k], bg[2][k])
        np.testing.assert_array_equal(batch.phi[k], one.phi)
        np.testing.assert_array_equal(tbatch.phi[k].cpu().numpy(), one.phi)
        assert (batch.iterations[k], batch.residual[k], batch.status[k]) == (one.iterations, one.residual, one.status)
    assert len(set(batch.iterations.tolist())) > 1                    # the maps of the batch stop at different counts


# ----------------------------------------------------------------------------- 5. phase_from_match

def test_phase_from_match_on_the_golden_match(I):
    from conftest import Case
    result = Case("A_small").expected(0)
    w = I.match_weight(result, "err")
    np.testing.assert_array_equal(w, ((result["err"] == 1) & np.isfinite(result["dx"]) & np.isfinite(result["dy"])).astype(float))
    assert 0 < w.sum() < w.size
    res = I.phase_from_match(result, scale=2.0, bias=(0.25, -0.5))
    assert res.status == I.CONVERGED and res.residual <= 1e-10
    by_hand = I.integrate(2.0 * (result["dx"] - 0.25), 2.0 * (result["dy"] + 0.5), w)
    np.testing.assert_array_equal(res.phi, by_hand.phi)
    assert res.iterations == by_hand.iterations
    wf = I.phase_from_match(result, weight="f")
    assert wf.status == I.CONVERGED and np.isfinite(wf.phi[E.diag(I.match_weight(result, "f")) > 0]).all()


# ----------------------------------------------------------------------------- 6. the full size

def test_full_size_map_with_holes_converges(I):
    """2028 x 2028 (the map size of the flagship workload) with the hole pattern, on device tensors; no dense reference."""
    import torch
    shape = (2028, 2028)
    i, j = np.meshgrid(np.linspace(0, 1, shape[0]), np.linspace(0, 1, shape[1]), indexing="ij")
    phi = 2.5 * np.sin(5.1 * i + 0.3) * np.cos(4.3 * j + 1.1)
    gx, gy = E.gradients(phi, 11, noise=1e-4)
    w = E.hole_weights(shape, 11)
    gx[w == 0] = np.nan
    gy[w == 0] = np.nan
    res = I.integrate(torch.from_numpy(gx).cuda(), torch.from_numpy(gy).cuda(), torch.from_numpy(w).cuda())
    print("2028 x 2028 with holes: %d iterations, residual %.2e, status %d" % (res.iterations, res.residual, res.status))
    assert res.status == I.CONVERGED and res.iterations < 500
    out = Integration_host(res)
    check_residual(out, gx, gy, w, 1e-10)


class Integration_host:
    def __init__(self, res):
        self.phi, self.residual, self.status, self.iterations = res.phi.cpu().numpy(), res.residual, res.status, res.iterations
