"""The three float64 block kernels (``umx_blk_gram_dev`` / ``umx_blk_combine_dev`` / ``umx_blk_scale_dev``, csrc/umx_rowblocks.h) on the
GPU, bit for bit against their NumPy statements in pdb2reaction_amd/rowblocks.py.  No weights are needed but for the curvature case.

Sizes: n in {3, 36, 255, 256, 257, 771} -- below one lane stride, at it, one past it, several strides with a ragged end, more than one
256-thread block of the element-wise kernels -- and p, q in {1, 3, 17, 64}, the last being the largest block taken."""
import numpy as np
import pytest
import torch

import hvp_cases as HC
import modes_cases as MC
from pdb2reaction_amd import modes as M
from pdb2reaction_amd.engine import UmxError

pytestmark = pytest.mark.gpu

NS = (3, 36, 255, 256, 257, 771)
PS = (1, 3, 17, 64)
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


def gram(e, x, y):
    g = torch.full((x.shape[0], y.shape[0]), 7.0, dtype=torch.float64, device=DEV)
    e.blk_gram_dev(x.shape[0], x.data_ptr(), y.shape[0], y.data_ptr(), x.shape[1], g.data_ptr(), stream=stream())
    return g.cpu().numpy()


@pytest.mark.parametrize("n", NS)
def test_each_entry_is_its_numpy_statement_bit_for_bit(eng, n):
    rng = np.random.default_rng(n)
    w_h = rng.standard_normal(n)
    w_h[::5] = 0.0                                                           # a freeze mask's zeros (and -0.0 * x)
    w = dev(w_h)
    for p in PS:
        x_h = MC.kernel_data(p, n, 100 * n + p)
        x = dev(x_h)
        # scale, out of place and in place
        y = torch.full_like(x, 7.0)
        eng.blk_scale_dev(p, x.data_ptr(), w.data_ptr(), n, y.data_ptr(), stream=stream())
        want = M.blk_scale(x_h, w_h)
        assert MC.same_bits(y.cpu().numpy(), want), ("scale", n, p)
        xi = x.clone()
        eng.blk_scale_dev(p, xi.data_ptr(), w.data_ptr(), n, xi.data_ptr(), stream=stream())
        assert MC.same_bits(xi.cpu().numpy(), want), ("scale in place", n, p)
        # gram of a block with itself: symmetric bit for bit
        gxx = gram(eng, x, x)
        assert MC.same_bits(gxx, M.blk_gram(x_h, x_h)) and MC.same_bits(gxx, gxx.T.copy()), ("gram(X, X)", n, p)
        for q in PS:
            y_h = MC.kernel_data(q, n, 100 * n + 10 * p + q + 1)
            yd = dev(y_h)
            assert MC.same_bits(gram(eng, x, yd), M.blk_gram(x_h, y_h)), ("gram", n, p, q)
            c_h = rng.standard_normal((p, q))
            c_h[0, 0] = -0.0
            c = dev(c_h)
            for subtract in (True, False):
                want = M.blk_combine(x_h, c_h, y_h, subtract)
                out = torch.full_like(yd, 7.0)
                eng.blk_combine_dev(p, x.data_ptr(), q, c.data_ptr(), n, yd.data_ptr(), subtract, out.data_ptr(), stream=stream())
                assert MC.same_bits(out.cpu().numpy(), want), ("combine", n, p, q, subtract)
                zi = yd.clone()                                              # Y aliasing Z
                eng.blk_combine_dev(p, x.data_ptr(), q, c.data_ptr(), n, zi.data_ptr(), subtract, zi.data_ptr(), stream=stream())
                assert MC.same_bits(zi.cpu().numpy(), want), ("combine in place", n, p, q, subtract)
            out = torch.full_like(yd, 7.0)                                   # no Z: the sum starts at 0.0
            eng.blk_combine_dev(p, x.data_ptr(), q, c.data_ptr(), n, 0, False, out.data_ptr(), stream=stream())
            assert MC.same_bits(out.cpu().numpy(), M.blk_combine(x_h, c_h, None, False)), ("combine without Z", n, p, q)


def test_refusals_come_before_any_launch_and_leave_the_outputs(eng):
    n = 36
    x, y, c, w = dev(MC.kernel_data(3, n, 1)), dev(MC.kernel_data(3, n, 2)), dev(np.ones((3, 3))), dev(np.ones(n))
    big = dev(np.ones((65, n)))
    g = torch.full((65, 65), 7.0, dtype=torch.float64, device=DEV)
    out = torch.full((65, n), 7.0, dtype=torch.float64, device=DEV)
    s = stream()
    bad = [
        lambda: eng.blk_gram_dev(0, x.data_ptr(), 3, y.data_ptr(), n, g.data_ptr(), stream=s),
        lambda: eng.blk_gram_dev(3, x.data_ptr(), -1, y.data_ptr(), n, g.data_ptr(), stream=s),
        lambda: eng.blk_gram_dev(3, x.data_ptr(), 3, y.data_ptr(), 0, g.data_ptr(), stream=s),
        lambda: eng.blk_gram_dev(65, big.data_ptr(), 3, y.data_ptr(), n, g.data_ptr(), stream=s),
        lambda: eng.blk_gram_dev(3, x.data_ptr(), 65, big.data_ptr(), n, g.data_ptr(), stream=s),
        lambda: eng.blk_gram_dev(3, 0, 3, y.data_ptr(), n, g.data_ptr(), stream=s),
        lambda: eng.blk_gram_dev(3, x.data_ptr(), 3, 0, n, g.data_ptr(), stream=s),
        lambda: eng.blk_combine_dev(0, x.data_ptr(), 3, c.data_ptr(), n, y.data_ptr(), True, out.data_ptr(), stream=s),
        lambda: eng.blk_combine_dev(3, x.data_ptr(), 0, c.data_ptr(), n, y.data_ptr(), True, out.data_ptr(), stream=s),
        lambda: eng.blk_combine_dev(3, x.data_ptr(), 3, c.data_ptr(), -5, y.data_ptr(), True, out.data_ptr(), stream=s),
        lambda: eng.blk_combine_dev(65, big.data_ptr(), 3, c.data_ptr(), n, y.data_ptr(), True, out.data_ptr(), stream=s),
        lambda: eng.blk_combine_dev(3, x.data_ptr(), 65, c.data_ptr(), n, y.data_ptr(), True, out.data_ptr(), stream=s),
        lambda: eng.blk_combine_dev(3, 0, 3, c.data_ptr(), n, y.data_ptr(), True, out.data_ptr(), stream=s),
        lambda: eng.blk_combine_dev(3, x.data_ptr(), 3, 0, n, y.data_ptr(), True, out.data_ptr(), stream=s),
        lambda: eng.blk_scale_dev(0, x.data_ptr(), w.data_ptr(), n, out.data_ptr(), stream=s),
        lambda: eng.blk_scale_dev(65, big.data_ptr(), w.data_ptr(), n, out.data_ptr(), stream=s),
        lambda: eng.blk_scale_dev(3, x.data_ptr(), w.data_ptr(), 0, out.data_ptr(), stream=s),
        lambda: eng.blk_scale_dev(3, x.data_ptr(), 0, n, out.data_ptr(), stream=s),
        lambda: eng.blk_scale_dev(3, 0, w.data_ptr(), n, out.data_ptr(), stream=s),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(UmxError) as err:
            call()
        assert err.value.status == -1, k                                     # UMX_ERR_ARG
    assert bool((g == 7.0).all()) and bool((out == 7.0).all())
    # Y aliasing X in combine: the whole block, and a part of it
    keep = x.cpu().numpy().copy()
    for target in (x.data_ptr(), x.data_ptr() + 8 * n):
        with pytest.raises(UmxError, match="overlaps d_x") as err:
            eng.blk_combine_dev(3, x.data_ptr(), 3, c.data_ptr(), n, y.data_ptr(), True, target, stream=s)
        assert err.value.status == -1
    for fn in (lambda: eng.blk_gram_dev(3, x.data_ptr(), 3, y.data_ptr(), n, 0, stream=s),
               lambda: eng.blk_combine_dev(3, x.data_ptr(), 3, c.data_ptr(), n, y.data_ptr(), True, 0, stream=s),
               lambda: eng.blk_scale_dev(3, x.data_ptr(), w.data_ptr(), n, 0, stream=s)):
        with pytest.raises(UmxError):
            fn()
    assert MC.same_bits(x.cpu().numpy(), keep)


def test_the_gram_diagonal_is_the_curvature_of_hvp(weights):
    from pdb2reaction_amd.engine import Engine

    c = HC.bases(weights)["swap"]
    dirs = HC.directions(len(c["z"]))
    e = Engine(0)
    try:
        e.load_weights(weights)
        e.set_system(c["z"], max_neigh=c["max_neigh"])
        hv, curv = e.hvp(c["x"], dirs, step=1e-3, return_curvature=True)
        d, h = dev(dirs.reshape(len(dirs), -1)), dev(hv.reshape(len(hv), -1))
        num, den = gram(e, d, h), gram(e, d, d)
        assert MC.same_bits(np.diag(num) / np.diag(den), curv)
    finally:
        e.close()
