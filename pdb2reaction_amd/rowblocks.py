"""Row-block algebra of the Hessian-free solvers (modes.py, dimer.py): float64 ROW vectors of length n = 3N, on the host or on a GPU.

A block is (p, n), p <= :data:`BLK_MAX`.  Six operations, each one kernel of csrc/umx_rowblocks.h and one NumPy function here:
``blk_gram`` / ``blk_combine`` / ``blk_scale`` mix the rows of a block through a small matrix or a weight vector; ``row_dot`` /
``row_axpby`` / ``row_absmax`` treat K rows as K independent vectors with scalars of their own.  The NumPy functions are the
SPECIFICATION of the kernels: the same products and sums in the same order, every product rounded before it is added, and the kernels
are held to them bit for bit (tests/test_gpu_modes_kernels.py, tests/test_gpu_rows_kernels.py).  The one order that matters, that of a
dot product, is written once (:func:`_lane_tree_sum`), so ``row_dot(x, y)`` is ``diag(blk_gram(x, y))`` by construction.

Two vector classes carry everything a solver does with rows but the Hessian-vector products:
  :class:`DeviceRows`  float64 torch tensors on an ``Engine``'s GPU; every operation is one engine entry (``umx_blk_*_dev``,
                       ``umx_row_*_dev``) on torch's current stream -- stream order is the only synchronisation; ``gram``, ``dot`` and
                       ``absmax`` read their small results back;
  :class:`HostRows`    NumPy arrays and the six functions.
Interface: ``put / get / rows / take / scatter / cat / vector``, ``gram / combine / scale``, ``dot / axpby / absmax``, ``project``.  A
solver's backend is one of the two plus its product adapter (``hvp`` and what goes with it), so a whole solver gives the same bits
through either backend on the same engine."""
from __future__ import annotations

import inspect
from typing import Callable, Optional

import numpy as np

BLK_MAX = 64                                   # rows of a block (umx_rowblocks.h): every small matrix read back stays <= 64 x 64 doubles
LANES = 256                                    # threads of the workgroup that adds one dot product


# ---- the six kernels' operation order, in NumPy ------------------------------------------------------------------------------------------
def _lane_tree_sum(prod: np.ndarray) -> np.ndarray:
    """The sum over the last axis as ``lane_tree_dot`` (umx_rowblocks.h) adds it: lane t of 256 adds the entries c = t, t + 256, ... in
    ascending order starting from 0.0, then the 256 partials are added in the tree s = 128, 64, ..., 1 (``part[t] += part[t + s]`` for
    t < s)."""
    lead, n = prod.shape[:-1], prod.shape[-1]
    strides = (n + LANES - 1) // LANES
    padded = np.zeros(lead + (strides * LANES,))       # a lane past the end adds nothing: x + 0.0 is x, and a partial is never -0.0
    padded[..., :n] = prod
    padded = padded.reshape(lead + (strides, LANES))
    part = np.zeros(lead + (LANES,))
    for r in range(strides):
        part = part + padded[..., r, :]
    s = LANES // 2
    while s > 0:
        part = part[..., :s] + part[..., s:2 * s]
        s >>= 1
    return part[..., 0].copy()


def blk_gram(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """``g[a][b] = sum_c x[a][c] * y[b][c]`` as ``k_blk_gram`` adds it (:func:`_lane_tree_sum`).  x (p,n), y (q,n) -> (p,q)."""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    g = np.empty((x.shape[0], y.shape[0]))
    for a in range(x.shape[0]):
        g[a] = _lane_tree_sum(x[a][None, :] * y)
    return g


def blk_combine(x: np.ndarray, c: np.ndarray, z: Optional[np.ndarray], subtract: bool) -> np.ndarray:
    """``y[j] = z[j] -+ sum_i c[i][j] * x[i]`` as ``k_blk_combine`` does it: acc = z[j] (0.0 without z), then i ascending,
    ``acc = fl(acc -+ fl(c * x))``.  x (p,n), c (p,q), z (q,n) or None -> (q,n)."""
    x, c = np.asarray(x, dtype=np.float64), np.asarray(c, dtype=np.float64)
    acc = np.zeros((c.shape[1], x.shape[1])) if z is None else np.array(z, dtype=np.float64)
    for i in range(x.shape[0]):
        t = c[i][:, None] * x[i][None, :]
        acc = acc - t if subtract else acc + t
    return acc


def blk_scale(x: np.ndarray, w: np.ndarray) -> np.ndarray:
    """``y[a][c] = fl(w[c] * x[a][c])`` (``k_blk_scale``)."""
    return np.asarray(w, dtype=np.float64)[None, :] * np.asarray(x, dtype=np.float64)


def row_dot(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """``out[r] = sum_c x[r][c] * y[r][c]`` as ``k_row_dot`` adds it (:func:`_lane_tree_sum`): the diagonal of :func:`blk_gram`."""
    return _lane_tree_sum(np.ascontiguousarray(x, dtype=np.float64) * np.ascontiguousarray(y, dtype=np.float64))


def row_axpby(a: np.ndarray, x: np.ndarray, b: Optional[np.ndarray] = None, y: Optional[np.ndarray] = None) -> np.ndarray:
    """``out[r][c] = fl(fl(a[r] * x[r][c]) + fl(b[r] * y[r][c]))``, or ``fl(a[r] * x[r][c])`` without ``(b, y)`` (``k_row_axpby``)."""
    if (b is None) != (y is None):
        raise ValueError("row_axpby: give both b and y, or neither")
    ax = np.asarray(a, dtype=np.float64)[:, None] * np.asarray(x, dtype=np.float64)
    return ax if y is None else ax + np.asarray(b, dtype=np.float64)[:, None] * np.asarray(y, dtype=np.float64)


def row_absmax(x: np.ndarray) -> np.ndarray:
    """``out[r] = max_c |x[r][c]|``, NaN when the row holds one (``k_row_absmax``)."""
    return np.max(np.abs(np.asarray(x, dtype=np.float64)), axis=1)


def takes(fn: Callable, name: str) -> bool:
    """Whether the callable ``fn`` has a parameter called ``name`` (an ``hvp`` that accepts ``base_forces``, say)."""
    try:
        return name in inspect.signature(fn).parameters
    except (TypeError, ValueError):
        return False


# ---- rows on the host and on the device ----------------------------------------------------------------------------------------------------
class HostRows:
    """Blocks are NumPy arrays (p, n)."""

    def put(self, a):
        return np.array(a, dtype=np.float64, ndmin=2)

    def get(self, b):
        return np.array(b, dtype=np.float64)

    def rows(self, b) -> int:
        return int(b.shape[0])

    def take(self, b, idx):
        return np.ascontiguousarray(b[list(idx)])

    def scatter(self, b, idx, sub):
        """A copy of ``b`` whose rows ``idx`` are those of ``sub``."""
        out = np.array(b)
        out[list(idx)] = sub
        return out

    def cat(self, blocks):
        return np.concatenate(blocks, axis=0)

    def vector(self, w):
        return np.array(w, dtype=np.float64)

    gram = staticmethod(blk_gram)
    combine = staticmethod(blk_combine)
    scale = staticmethod(blk_scale)
    dot = staticmethod(row_dot)
    axpby = staticmethod(row_axpby)
    absmax = staticmethod(row_absmax)

    def project(self, qs, u):
        """Row i of ``u`` minus its components along the rows of ``qs[i]`` (None: untouched): ``blk_gram`` + ``blk_combine`` per row."""
        out = np.array(u)
        for i, q in enumerate(qs):
            if q is not None:
                out[i:i + 1] = blk_combine(q, blk_gram(q, u[i:i + 1]), u[i:i + 1], True)
        return out


class DeviceRows:
    """Blocks are float64 torch tensors (p, n) on the engine's GPU; every operation is one engine entry on torch's current stream (stream
    order is the only synchronisation, as in ``parallel.EngineStringEvaluator.hvp``).  Small results (``gram``, ``dot``, ``absmax``) are
    read back; small operands (``combine``'s C, ``axpby``'s a and b) are sent."""

    def __init__(self, engine):
        import torch

        self.torch, self.engine = torch, engine
        self.dev = torch.device("cuda", int(engine.device))

    def _stream(self) -> int:
        return self.torch.cuda.current_stream(self.dev).cuda_stream

    def empty(self, *shape, dtype=None):
        return self.torch.empty(*shape, dtype=self.torch.float64 if dtype is None else dtype, device=self.dev)

    def put(self, a, ndmin: int = 2):
        return self.torch.as_tensor(np.array(a, dtype=np.float64, ndmin=ndmin), device=self.dev).contiguous()

    def get(self, b):
        return b.cpu().numpy()

    def rows(self, b) -> int:
        return int(b.shape[0])

    def take(self, b, idx):
        return b[list(idx)].contiguous()

    def scatter(self, b, idx, sub):
        out = b.clone()
        out[list(idx)] = sub
        return out

    def cat(self, blocks):
        return self.torch.cat(blocks, dim=0).contiguous()

    def vector(self, w):
        return self.put(w, ndmin=0)

    def _gram(self, p, d_x, q, d_y, n):
        g = self.empty(p, q)
        self.engine.blk_gram_dev(p, d_x, q, d_y, n, g.data_ptr(), stream=self._stream())
        return g

    def gram(self, x, y) -> np.ndarray:
        return self._gram(x.shape[0], x.data_ptr(), y.shape[0], y.data_ptr(), x.shape[1]).cpu().numpy()

    def combine(self, x, c, z, subtract):
        c = self.put(c)
        y = self.empty(c.shape[1], x.shape[1])
        self.engine.blk_combine_dev(x.shape[0], x.data_ptr(), c.shape[1], c.data_ptr(), x.shape[1], 0 if z is None else z.data_ptr(), subtract,
                                    y.data_ptr(), stream=self._stream())
        return y

    def scale(self, x, w):
        y = self.torch.empty_like(x)
        self.engine.blk_scale_dev(x.shape[0], x.data_ptr(), w.data_ptr(), x.shape[1], y.data_ptr(), stream=self._stream())
        return y

    def dot(self, x, y) -> np.ndarray:
        out = self.empty(x.shape[0])
        self.engine.row_dot_dev(x.shape[0], x.data_ptr(), y.data_ptr(), x.shape[1], out.data_ptr(), stream=self._stream())
        return out.cpu().numpy()

    def axpby(self, a, x, b=None, y=None):
        if (b is None) != (y is None):
            raise ValueError("row_axpby: give both b and y, or neither")
        ad = self.vector(a)
        bd = None if b is None else self.vector(b)
        out = self.torch.empty_like(x)
        self.engine.row_axpby_dev(x.shape[0], ad.data_ptr(), x.data_ptr(), 0 if bd is None else bd.data_ptr(), 0 if y is None else y.data_ptr(),
                                  x.shape[1], out.data_ptr(), stream=self._stream())
        return out

    def absmax(self, x) -> np.ndarray:
        out = self.empty(x.shape[0])
        self.engine.row_absmax_dev(x.shape[0], x.data_ptr(), x.shape[1], out.data_ptr(), stream=self._stream())
        return out.cpu().numpy()

    def project(self, qs, u):
        """As :meth:`HostRows.project`; a row's Gram column stays on the device as its combine's C -- row pointer offsets, no read-back."""
        n = int(u.shape[1])
        out = u.clone()
        for i, q in enumerate(qs):
            if q is not None:
                r = int(q.shape[0])
                row_in, row_out = u.data_ptr() + 8 * n * i, out.data_ptr() + 8 * n * i
                g = self._gram(r, q.data_ptr(), 1, row_in, n)
                self.engine.blk_combine_dev(r, q.data_ptr(), 1, g.data_ptr(), n, row_in, True, row_out, stream=self._stream())
        return out
