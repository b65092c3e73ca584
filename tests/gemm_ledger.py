"""Which rows of the plane-GEMM dispatch table (`pl_kernels`, csrc/umx_launch.h) the link tests launch -- read from the engine, never restated.

`umx_debug_fetch("gemm:table")` lists the table, one "fam cplx wide ls al half" per row; `"gemm:launches"` lists the gemm_pl launches of the
most recent evaluation's last chunk, "fwd|rev fam cplx wide ls al half M N K blocks" per launch.  tests/test_gpu_forward_gemm_links.py's
ledger test forms the union of the keys its own cases launched and checked with the keys below, and requires it to BE the table.
tests/test_gpu_reverse_links.py and tests/test_gpu_forward_links.py assert that they launch exactly what is written here for them.  Only what
those files compare with a reference counts for the ledger: the REVERSE launches of test_gpu_reverse_links (conv^T and fc3^T of every mode)
and the forward launches of test_gpu_forward_links' `split` mode (its fp16 GEMM check); a forward launch of a run that only looks at the
reverse pass holds nothing."""
from collections import namedtuple

import numpy as np

Launch = namedtuple("Launch", "fwd key M N K blocks")


def _text(eng, name):
    return eng.debug_fetch(name, dtype=np.uint8).tobytes().decode()


def table(eng):
    """the rows of pl_kernels as a list of key strings (a list: a duplicated row shows)"""
    return [ln for ln in _text(eng, "gemm:table").split("\n") if ln]


def launches(eng):
    out = []
    for ln in _text(eng, "gemm:launches").split("\n"):
        if ln:
            f = ln.split()
            assert len(f) == 11 and f[0] in ("fwd", "rev"), ln
            out.append(Launch(f[0] == "fwd", " ".join(f[1:7]), int(f[7]), int(f[8]), int(f[9]), int(f[10])))
    return out


def keys(eng, fwd=None):
    """the keys of the logged launches; fwd = True / False: of the forward / reverse pass only"""
    return {x.key for x in launches(eng) if fwd is None or x.fwd == fwd}


def field(key, name):
    f = key.split()
    return f[0] if name == "fam" else int(f[("cplx", "wide", "ls", "al", "half").index(name) + 1])


# ---- what the two older link files launch, per (mode, size) of their cases (read from "gemm:launches" on the MI355X) ------------------
def _q(*f):
    return "Q_BF16 %d %d %d %d %d" % f


_PL3 = {"PL3 0 0 0 0 0", "PL3_ROWS 0 0 0 0 0"}
# reverse launches (forces on): bf16x3 -- quad-row conv^T (half-height where K >= 256), three-plane fc3^T; split-bf16 -- two-plane PL products
KEYS_REVERSE_LINKS = {
    ("bf16x3", "S"): _PL3 | {_q(0, 0, 0, 0, 1), _q(1, 0, 0, 0, 0), _q(1, 0, 0, 0, 1)},
    ("bf16x3", "L"): _PL3 | {_q(0, 0, 0, 0, 1), _q(0, 1, 0, 0, 1), _q(1, 1, 0, 0, 0), _q(1, 1, 0, 0, 1)},
    ("fp32", "S"): set(), ("fp32", "L"): set(),
    ("split-bf16", "S"): {"PL2_M16 0 0 0 0 0", "PL2_M16 1 0 0 0 0", "PL2_M32 0 0 0 0 0"},
    ("split-bf16", "L"): {"PL2_M16 0 0 0 0 0", "PL2_M32 0 0 0 0 0", "PL2_WIDE 0 1 0 0 0", "PL2_WIDE 1 1 0 0 0"},
}
# forward launches (energy only); the ledger counts the `split` rows, whose GEMM that file holds
_FWD_NARROW = {_q(0, 0, 1, 1, 0), _q(0, 1, 1, 1, 0), _q(1, 0, 0, 0, 0), _q(1, 0, 0, 0, 1)}
KEYS_FORWARD_LINKS = {
    ("bf16x3", "T1"): _FWD_NARROW, ("bf16x3", "S"): _FWD_NARROW,
    ("bf16x3", "L"): {_q(0, 0, 1, 1, 0), _q(0, 1, 1, 1, 0), _q(1, 1, 0, 0, 0), _q(1, 1, 0, 0, 1)},
    ("fp32", "T1"): set(), ("fp32", "S"): set(), ("fp32", "L"): set(),
    ("split", "T1"): {"Q_F16 0 0 0 0 0", "Q_F16 1 0 0 0 0"}, ("split", "S"): {"Q_F16 0 0 0 0 0", "Q_F16 1 0 0 0 0"},
    ("split", "L"): {"Q_F16 0 0 0 0 0", "Q_F16 0 1 0 0 0", "Q_F16 1 1 0 0 0"},
}


def held_elsewhere():
    """the rows those two files launch AND compare with a reference"""
    return set().union(*KEYS_REVERSE_LINKS.values(), *(v for (mode, _), v in KEYS_FORWARD_LINKS.items() if mode == "split"))
