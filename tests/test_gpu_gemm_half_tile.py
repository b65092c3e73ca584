"""The half-height split-precision GEMMs (umx_gemm_q.h MW = 2: 128-row tiles, two 4-wave workgroups per CU) give the bits of the 256-row forms.

A tile's height enters no output element's arithmetic -- same per-wave tile, same k order, same fold points -- so an engine with the half-height
forms forced on everywhere (`UMX_GEMM_HALF=3`: every Q_BF16 product, both passes) must reproduce an engine with them off (`UMX_GEMM_HALF=0`) bit
for bit: energies, forces and the captures behind every switched GEMM.  What can go wrong is the row tiling, so the systems are chosen by their
directed-edge count M.  An open chain of n atoms 4.5 A apart (cutoff 6 A; jitter below 0.5 A per coordinate, so only chain neighbours are within
the cutoff) has exactly M = 2 n - 2 directed edges:

    n = 20   M =   38   less than one 64-row wave tile; M % 4 = 2
    n = 64   M =  126   just under one 128-row tile (two 64-edge complex tiles); M % 4 = 2
    n = 65   M =  128   exactly one tile
    n = 66   M =  130   one tile and two rows; M % 4 = 2
    n = 130  M =  258   just over two tiles (just over one 256-row tile of the full-height form); M % 4 = 2
    n = 700  M = 1398   11 plain / 22 complex row tiles: more than 8, no multiple of 8 -- blockIdx -> (XCD, row tile) wraps with a remainder
"""
import os

import numpy as np
import pytest
import torch

from pdb2reaction_amd import weights as W

pytestmark = pytest.mark.gpu

CAPTURES = ["rad.deg"] + [f"{name}.{i}" for i in range(W.NUM_LAYERS) for name in ("rad", "hg", "msg", "g_hid", "g_y1", "g_a2")]


def _chain(n, images=1, seed=0):
    rng = np.random.default_rng(1000 * n + seed)
    z = rng.choice(np.array([1, 6, 7, 8]), size=n)
    pos = np.zeros((images, n, 3))
    pos[:, :, 0] = 4.5 * np.arange(n)[None, :]
    pos += rng.uniform(-1.0, 1.0, size=pos.shape) * np.array([0.3, 0.5, 0.5])
    return z, pos.astype(np.float32)


def _engines(precision, **switches):
    from pdb2reaction_amd.engine import Engine

    w = W.make_synthetic_weights(1)
    old = {k: os.environ.get(k) for k in ("UMX_GEMM_HALF", *switches)}
    made = []
    try:
        os.environ.update(switches)
        for half in ("0", "3"):                  # the switches are read when the engine is created
            os.environ["UMX_GEMM_HALF"] = half
            eng = Engine(0, precision=precision)
            made.append(eng)
            eng.load_weights(w)
            eng.debug_keep(True)
    except BaseException:
        for eng in made:
            eng.close()
        raise
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return made


@pytest.fixture(scope="module")
def engines():
    pair = _engines("bf16x3")
    yield pair
    for eng in pair:
        eng.close()


def _evaluate(eng, z, pos, captures=True):
    eng.set_system(z)
    e, f = eng.energy_forces(pos)
    out = {"E": e.copy(), "F": f.copy()}
    if captures:
        for name in CAPTURES:
            out[name] = eng.debug_fetch(name).copy()
    return out, eng.graph_stats()[0]


def _same(a, b):
    return torch.equal(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))


def _compare(off, on, label):
    assert np.isfinite(off["E"]).all() and np.isfinite(off["F"]).all(), label
    differ = [name for name in off if not _same(off[name], on[name])]
    assert not differ, f"{label}: the half-height forms differ from the full-height ones in {differ}"


@pytest.mark.parametrize("n,edges", [(20, 38), (64, 126), (65, 128), (66, 130), (130, 258), (700, 1398)])
def test_half_height_tiles_bit_for_bit(engines, n, edges):
    z, pos = _chain(n)
    off, ne_off = _evaluate(engines[0], z, pos)
    on, ne_on = _evaluate(engines[1], z, pos)
    assert ne_off == edges and ne_on == edges, f"the chain of {n} atoms has {ne_off} / {ne_on} directed edges, not {edges}"
    assert off["rad.deg"].size == edges * 3 * W.SPHERE_CHANNELS and off["hg.0"].size % edges == 0
    _compare(off, on, f"M = {edges}")


@pytest.fixture(scope="module")
def engines_ls_al():
    """The complex products with LS and aligned planes together (UMX_LOW_SEP=2, UMX_ALIGN_PLANES=1), full- and half-height."""
    pair = _engines("bf16x3", UMX_LOW_SEP="2", UMX_ALIGN_PLANES="1")
    yield pair
    for eng in pair:
        eng.close()


@pytest.mark.parametrize("n,edges", [(66, 130), (130, 258)])
def test_half_height_tiles_bit_for_bit_ls_aligned(engines_ls_al, n, edges):
    z, pos = _chain(n)
    off, ne_off = _evaluate(engines_ls_al[0], z, pos)
    on, ne_on = _evaluate(engines_ls_al[1], z, pos)
    assert ne_off == edges and ne_on == edges
    _compare(off, on, f"LOW_SEP = 2, ALIGN_PLANES = 1, M = {edges}")


def test_half_height_tiles_batch_independence(engines):
    """Two images in one batch (M = 2 x 78: the second image starts in the middle of a tile) against the same images evaluated alone."""
    eng = engines[1]
    z, pos = _chain(40, images=2)
    both, ne = _evaluate(eng, z, pos, captures=False)
    assert ne == 2 * 78
    for k in range(2):
        alone, ne1 = _evaluate(eng, z, pos[k:k + 1], captures=False)
        assert ne1 == 78
        assert _same(alone["E"][0], both["E"][k]) and _same(alone["F"][0], both["F"][k]), f"image {k} differs between the batch and alone"
    full, _ = _evaluate(engines[0], z, pos, captures=False)
    _compare(full, both, "batch of two images")


def test_half_height_tiles_bit_for_bit_split_bf16():
    """split-bf16: the forward pass on the same Q_BF16 kernels, the reverse pass on the two-plane PL kernels (which have no half-height form)."""
    pair = _engines("split-bf16")
    try:
        z, pos = _chain(66)
        off, ne_off = _evaluate(pair[0], z, pos)
        on, ne_on = _evaluate(pair[1], z, pos)
        assert ne_off == 130 and ne_on == 130
        _compare(off, on, "split-bf16, M = 130")
    finally:
        for eng in pair:
            eng.close()
