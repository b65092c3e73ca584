"""Recompute plans without a GPU: the ABI symbols, the keyword plumbing down to every engine (fake engines, as in
``test_local_pool_cpu.py``), and the planner's size arithmetic (``umx_workspace_bytes`` needs no device with a NULL engine)."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

from pdb2reaction_amd import engine as E, parallel as P
from test_local_pool_cpu import FakeEngine

U = importlib.import_module("pdb2reaction_amd.uma_pysis")
A = importlib.import_module("pdb2reaction_amd.ase_calculator")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# rows of float32 per directed edge (csrc/umx_common.h): the radial MLP's two hidden pre-activations, its output, conv 1's [gate | hidden],
# the message; four layers, plus the edge-degree link (its own h1pre / h2pre and 3 x 128 radial rows)
RH, RAD, HG, ROW, C, NL = 128, 1536, 1408, 1152, 128, 4


def test_symbols_in_header_library_and_export_list():
    txt = open(os.path.join(ROOT, "include", "umx.h")).read()
    lib = E.load_library()
    for sym in ("umx_set_recompute", "umx_last_recompute", "umx_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % sym, re.sub(r"/\*.*?\*/", "", txt, flags=re.S)), sym
        assert sym in E.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert "UMX_RECOMPUTE" in txt and lib.umx_abi_version() == 10          # additive: no version bump
    assert callable(E.Engine.set_recompute) and callable(E.Engine.last_recompute)


def _stored_acts(ne):
    return 4 * ne * ((NL + 1) * 2 * RH + 3 * C + NL * (RAD + HG + ROW))


def _slot(ne):
    return 4 * ne * (2 * RH + RAD + HG + ROW)


@pytest.mark.parametrize("nn,ne", [(97, 4096), (300, 16640), (2000, 131072), (20000, 1600000)])
def test_one_piece_recompute_carve_is_smaller_by_the_per_layer_activations(nn, ne):
    """ne a multiple of 64: every buffer is then a multiple of the arena's 256-byte alignment and the difference is exact."""
    stored, rc = E.workspace_bytes(nn, ne, 0, 0), E.workspace_bytes(nn, ne, 0, 1)
    assert stored - rc == _stored_acts(ne) - _slot(ne)
    assert stored - rc == 4 * ne * (NL * 2 * RH + 3 * C + (NL - 1) * (RAD + HG + ROW))       # the same thing, buffer by buffer
    assert E.workspace_bytes(0, ne, 0, 1) < 0.56 * E.workspace_bytes(0, ne, 0, 0)             # ~66 of ~120 KB per edge


@pytest.mark.parametrize("parts", [2, 3, 5, 16])
def test_partitioned_recompute_shares_one_slot(parts):
    nn, ne = 300, 64 * parts * 40
    stored, rc = E.workspace_bytes(nn, ne, parts, 0), E.workspace_bytes(nn, ne, parts, 1)
    per = ne // parts
    # stored: every partition keeps the activations of ITS edges; recompute: one slot for the largest partition
    assert stored - rc == _stored_acts(ne) - _slot(per)
    # node-level state and the small per-edge buffers stay per partition in both: the persistent part does not shrink with more partitions
    node_and_graph = E.workspace_bytes(nn, 0, 0, 1)
    assert rc > parts * node_and_graph
    # what 2..16 partitions are for: per-edge memory of a recompute plan falls with P, a stored plan's does not fall below its activations
    assert rc - parts * node_and_graph < (stored - parts * node_and_graph) / parts * 1.01 + 4 * ne * 128
    assert stored > _stored_acts(ne)


def test_arithmetic_argument_checks():
    for bad in ((10, 10, 1, 0), (10, 10, 17, 0), (-1, 10, 0, 0), (10, -1, 0, 1)):
        with pytest.raises(ValueError):
            E.workspace_bytes(*bad)
    assert E.workspace_bytes(10, 0, 0, 0) == E.workspace_bytes(10, 0, 0, 1)                   # no edges: nothing to recompute


# ---- keyword plumbing ---------------------------------------------------------------------------------------------------------------
class RecEngine(FakeEngine):
    made = []

    def __init__(self, device=0, precision=None):
        super().__init__(device, precision)
        self.recompute = None
        RecEngine.made.append(self)

    def set_recompute(self, mode):
        self.recompute = int(mode)

    def last_recompute(self):
        return 1 if self.recompute == 2 else 0


@pytest.fixture
def made(monkeypatch):
    RecEngine.made = []
    monkeypatch.setattr(E, "Engine", RecEngine)
    return RecEngine.made


def test_pool_hands_the_mode_to_every_engine(made):
    pool = P.LocalEnginePool.create([0, 1, 2], {"w": 1}, engine_factory=RecEngine, recompute=1, peer_sum=lambda *a: None,
                                    tensor_device=lambda e: torch.device("cpu"))
    assert [e.recompute for e in made] == [1, 1, 1] and pool.recompute == 1
    pool.set_recompute(2)
    assert [e.recompute for e in made] == [2, 2, 2] and pool.last_recompute() == 1
    # mode 2 is a one-GPU plan: a single image goes to engine 0 alone, never through umx_gp_begin
    pool.set_system([8, 1, 1, 1])
    pool.energy_forces(np.zeros((1, 4, 3), np.float32))
    assert pool.last_route == "single" and all(not e.gp_calls for e in made)
    del made[:]
    P.LocalEnginePool.create([0, 1], {"w": 1}, engine_factory=RecEngine, peer_sum=lambda *a: None, tensor_device=lambda e: torch.device("cpu"))
    assert [e.recompute for e in made] == [None, None]                                         # default: the engines' own UMX_RECOMPUTE


def test_core_and_calculator_keywords(made, monkeypatch):
    monkeypatch.delenv("UMX_LOCAL_DEVICES", raising=False)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 1)
    core = U.UMAcore(["O", "H", "H"], model="synthetic", recompute=2)
    assert [e.recompute for e in made] == [2]
    core.close()
    del made[:]
    U.UMAcore(["O", "H", "H"], model="synthetic").close()
    assert [e.recompute for e in made] == [None]                                               # untouched: the environment decides
    del made[:]
    monkeypatch.setenv("UMX_LOCAL_DEVICES", "0,0")
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda d=None: (64 << 30, 64 << 30), raising=False)
    core = U.UMAcore(["O", "H", "H"], model="synthetic", workers=2, recompute=1)
    assert [e.recompute for e in made] == [1, 1] and core._pool.recompute == 1
    core.close()
    del made[:]
    monkeypatch.delenv("UMX_LOCAL_DEVICES")
    calc = U.uma_pysis(model="synthetic", recompute=1)                                         # through **kwargs, like precision=
    assert calc._core_kw["recompute"] == 1 and list(U.CALC_KW).count("recompute") == 0         # the reference's keyword table is as it was
    calc.get_energy(["H", "H"], [0, 0, 0, 0, 0, 1.4])
    assert [e.recompute for e in made] == [1]
    with pytest.raises(ValueError, match="recompute"):
        U.uma_pysis(model="synthetic", recompute=3)
    assert A.UMXCalculator(model="synthetic", recompute=2).recompute == 2
    with pytest.raises(ValueError, match="recompute"):
        A.UMXCalculator(model="synthetic", recompute="yes")
