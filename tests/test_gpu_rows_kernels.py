"""The three float64 row kernels (``umx_row_dot_dev`` / ``umx_row_axpby_dev`` / ``umx_row_absmax_dev``, csrc/umx_rowblocks.h) on the GPU, bit
for bit against their NumPy statements in pdb2reaction_amd/rowblocks.py.  No weights are needed.

Sizes: n in {3, 36, 255, 256, 257, 771} -- below one lane stride, at it, one past it, several strides with a ragged end, more than one
256-thread block of the element-wise kernel -- and k in {1, 3, 17, 64}, the last being the largest batch taken."""
import numpy as np
import pytest
import torch

import modes_cases as MC
from pdb2reaction_amd import dimer as D
from pdb2reaction_amd.engine import UmxError

pytestmark = pytest.mark.gpu

NS = (3, 36, 255, 256, 257, 771)
KS = (1, 3, 17, 64)
DEV = "cuda:0"


@pytest.fixture(scope="module")
def eng():
    from pdb2reaction_amd.engine import Engine

    e = Engine(0)                                                            # no weights, no system: the entries need neither
    yield e
    e.close()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)


def stream():
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


def dot(e, x, y):
    out = torch.full((x.shape[0],), 7.0, dtype=torch.float64, device=DEV)
    e.row_dot_dev(x.shape[0], x.data_ptr(), y.data_ptr(), x.shape[1], out.data_ptr(), stream=stream())
    return out.cpu().numpy()


def absmax(e, x):
    out = torch.full((x.shape[0],), 7.0, dtype=torch.float64, device=DEV)
    e.row_absmax_dev(x.shape[0], x.data_ptr(), x.shape[1], out.data_ptr(), stream=stream())
    return out.cpu().numpy()


def axpby(e, a, x, b, y, out):
    e.row_axpby_dev(x.shape[0], a.data_ptr(), x.data_ptr(), 0 if b is None else b.data_ptr(), 0 if y is None else y.data_ptr(), x.shape[1],
                    out.data_ptr(), stream=stream())
    return out.cpu().numpy()


@pytest.mark.parametrize("n", NS)
def test_each_entry_is_its_numpy_statement_bit_for_bit(eng, n):
    rng = np.random.default_rng(n)
    for k in KS:
        x_h, y_h = MC.kernel_data(k, n, 100 * n + k), MC.kernel_data(k, n, 100 * n + k + 50)
        a_h, b_h = rng.standard_normal(k), rng.standard_normal(k)
        a_h[0] = -0.0                                                        # a row scaled by a negative zero
        x, y, a, b = dev(x_h), dev(y_h), dev(a_h), dev(b_h)
        # dot: the statement, the block kernel's diagonal, a row with itself
        got = dot(eng, x, y)
        assert MC.same_bits(got, D.row_dot(x_h, y_h)), ("dot", n, k)
        g = torch.full((k, k), 7.0, dtype=torch.float64, device=DEV)
        eng.blk_gram_dev(k, x.data_ptr(), k, y.data_ptr(), n, g.data_ptr(), stream=stream())
        assert MC.same_bits(got, np.diag(g.cpu().numpy()).copy()), ("dot against blk_gram's diagonal", n, k)
        assert MC.same_bits(dot(eng, x, x), D.row_dot(x_h, x_h)), ("dot(X, X)", n, k)
        # axpby: out of place, in place on either operand, and without (b, y)
        want = D.row_axpby(a_h, x_h, b_h, y_h)
        assert MC.same_bits(axpby(eng, a, x, b, y, torch.full_like(x, 7.0)), want), ("axpby", n, k)
        xi = x.clone()
        assert MC.same_bits(axpby(eng, a, xi, b, y, xi), want), ("axpby in place on x", n, k)
        yi = y.clone()
        assert MC.same_bits(axpby(eng, a, x, b, yi, yi), want), ("axpby in place on y", n, k)
        want = D.row_axpby(a_h, x_h)
        assert MC.same_bits(axpby(eng, a, x, None, None, torch.full_like(x, 7.0)), want), ("a x", n, k)
        xi = x.clone()
        assert MC.same_bits(axpby(eng, a, xi, None, None, xi), want), ("a x in place", n, k)
        assert MC.same_bits(axpby(eng, a, x, a, x, torch.full_like(x, 7.0)), D.row_axpby(a_h, x_h, a_h, x_h)), ("axpby with y = x", n, k)
        # absmax: the statement; a NaN in one row is that row's result alone
        assert MC.same_bits(absmax(eng, x), D.row_absmax(x_h)), ("absmax", n, k)
        z_h = x_h.copy()
        z_h[k // 2, n - 1] = np.nan
        z_h[0, 0] = -np.inf if k > 1 else z_h[0, 0]
        got, want = absmax(eng, dev(z_h)), D.row_absmax(z_h)
        assert np.isnan(got[k // 2]) and np.array_equal(np.isnan(got), np.isnan(want)), ("absmax NaN", n, k)
        assert MC.same_bits(got[~np.isnan(got)], want[~np.isnan(want)]), ("absmax beside a NaN row", n, k)


def test_refusals_come_before_any_launch_and_leave_the_outputs(eng):
    n = 36
    x, y, a, b = dev(MC.kernel_data(3, n, 1)), dev(MC.kernel_data(3, n, 2)), dev(np.ones(3)), dev(np.ones(3))
    big, big_a = dev(np.ones((65, n))), dev(np.ones(65))
    vec = torch.full((65,), 7.0, dtype=torch.float64, device=DEV)
    out = torch.full((65, n), 7.0, dtype=torch.float64, device=DEV)
    s = stream()
    X, Y, A, B, V, O = x.data_ptr(), y.data_ptr(), a.data_ptr(), b.data_ptr(), vec.data_ptr(), out.data_ptr()
    bad = [
        (lambda: eng.row_dot_dev(0, X, Y, n, V, stream=s), "k = 0"),
        (lambda: eng.row_dot_dev(3, X, Y, 0, V, stream=s), "n = 0"),
        (lambda: eng.row_dot_dev(-2, X, Y, n, V, stream=s), "k = -2"),
        (lambda: eng.row_dot_dev(65, big.data_ptr(), big.data_ptr(), n, V, stream=s), "k = 65"),
        (lambda: eng.row_dot_dev(3, 0, Y, n, V, stream=s), "d_x"),
        (lambda: eng.row_dot_dev(3, X, 0, n, V, stream=s), "d_y"),
        (lambda: eng.row_axpby_dev(0, A, X, B, Y, n, O, stream=s), "k = 0"),
        (lambda: eng.row_axpby_dev(3, A, X, B, Y, -1, O, stream=s), "n = -1"),
        (lambda: eng.row_axpby_dev(65, big_a.data_ptr(), big.data_ptr(), 0, 0, n, O, stream=s), "k = 65"),
        (lambda: eng.row_axpby_dev(3, 0, X, B, Y, n, O, stream=s), "d_a"),
        (lambda: eng.row_axpby_dev(3, A, 0, B, Y, n, O, stream=s), "d_x"),
        (lambda: eng.row_axpby_dev(3, A, X, 0, Y, n, O, stream=s), "d_b is NULL"),      # exactly one of the pair
        (lambda: eng.row_axpby_dev(3, A, X, B, 0, n, O, stream=s), "d_y is NULL"),
        (lambda: eng.row_absmax_dev(0, X, n, V, stream=s), "k = 0"),
        (lambda: eng.row_absmax_dev(3, X, 0, V, stream=s), "n = 0"),
        (lambda: eng.row_absmax_dev(65, big.data_ptr(), n, V, stream=s), "k = 65"),
        (lambda: eng.row_absmax_dev(3, 0, n, V, stream=s), "d_x"),
    ]
    for i, (call, names) in enumerate(bad):
        with pytest.raises(UmxError, match=names) as err:
            call()
        assert err.value.status == -1, i                                     # UMX_ERR_ARG
    assert bool((vec == 7.0).all()) and bool((out == 7.0).all())
    # outputs that overlap an input, and a missing output: the inputs keep their bits
    keep_x, keep_y = x.cpu().numpy().copy(), y.cpu().numpy().copy()
    for call, names in ((lambda: eng.row_dot_dev(3, X, Y, n, X + 8 * 5, stream=s), "overlaps d_x"),
                        (lambda: eng.row_dot_dev(3, X, Y, n, Y, stream=s), "overlaps d_y"),
                        (lambda: eng.row_absmax_dev(3, X, n, X + 8 * (3 * n - 1), stream=s), "overlaps d_x"),
                        (lambda: eng.row_axpby_dev(3, A, X, B, Y, n, X + 8 * n, stream=s), "overlaps d_x"),        # shifted by a row: a race
                        (lambda: eng.row_axpby_dev(3, A, X, B, Y, n, Y + 8, stream=s), "overlaps d_y"),
                        (lambda: eng.row_dot_dev(3, X, Y, n, 0, stream=s), "d_out"),
                        (lambda: eng.row_axpby_dev(3, A, X, B, Y, n, 0, stream=s), "d_out"),
                        (lambda: eng.row_absmax_dev(3, X, n, 0, stream=s), "d_out")):
        with pytest.raises(UmxError, match=names) as err:
            call()
        assert err.value.status == -1
    torch.cuda.synchronize()
    assert MC.same_bits(x.cpu().numpy(), keep_x) and MC.same_bits(y.cpu().numpy(), keep_y)
