"""Pack plan of the fused eval-mode weights: what ``FusedPWCLONet`` packed, recorded so that one kernel can redo it.

While ``FusedPWCLONet.__init__`` runs, every ``fused.pack_layer`` call leaves one ``PackJob`` here: the ``_ConvBlock`` the
folded tensors came from, the column range and the bias switch that survived the slices / paddings between
``fold_conv_bn`` and ``pack_layer`` (carried as a ``_pack_src`` attribute on the folded tensors), the layout arguments,
and -- followed through every ``torch.cat`` of the constructors -- the buffer and offset the packed layer ended up at.
``PackPlan`` turns the jobs into the device table of csrc/pack_refresh.hip (include/pwclo_ops.h: PwcloPackJob) and
``refresh()`` launches that kernel: the packed buffers are rewritten in place from the live module tensors, bit for bit
what a fresh ``FusedPWCLONet`` would hold, with no buffer address and no Python object changed.
"""
import contextlib
import ctypes

import torch

from . import _lib

_recorder = None


class PackJob:
    """One packed layer.  ``layer``: the source ``_ConvBlock`` (``name``: its qualified name in the network);
    ``col0``: first column of the folded (Cout, Cin) matrix the layer uses, ``phys_map`` is relative to it;
    ``use_bias``: folded bias (True) or zeros; ``cout`` / ``cin``: the conv weight's own shape (rows >= cout of the
    16 * ``nbo`` packed rows are padding); ``nbi``, ``fmt`` (the tile format really used: odd ``nbi`` stays fp32),
    ``kmajor``: ``pack_layer``'s layout; ``dst`` / ``dst_off``: the packed buffer and the layer's first float in it."""

    def __init__(self, layer, col0, use_bias, phys_map, nbo, fmt, kmajor, out):
        conv = layer.conv
        self.layer, self.name = layer, None
        self.col0, self.use_bias = int(col0), bool(use_bias)
        self.cout, self.cin = int(conv.weight.shape[0]), int(conv.weight.numel() // conv.weight.shape[0])
        self.phys_map = [int(c) for c in phys_map]
        self.nbo, self.nbi, self.fmt, self.kmajor = int(nbo), len(self.phys_map) // 16, int(fmt), bool(kmajor)
        self.dst, self.dst_off = out, 0
        assert self.col0 >= 0 and self.col0 + max(self.phys_map) < self.cin and min(self.phys_map) >= -1
        assert self.fmt == 0 or self.nbi % 2 == 0
        assert not self.kmajor or (self.cout <= 16 and self.nbo == 1)

    @property
    def tiles(self):
        """Grid tiles of the job: its operand tiles and one for the bias vector."""
        return self.nbo * (self.nbi if self.fmt == 0 else self.nbi // 2) + 1

    @property
    def floats(self):
        per_tile = 768 if self.fmt == 1 else 256
        return (self.tiles - 1) * per_tile + 16 * self.nbo

    def tensors(self):
        """The live source tensors, read from the module at call time: dict with ``w``, ``conv_bias`` and the four
        BatchNorm tensors (None where the layer has none) and ``eps``."""
        conv = self.layer.conv
        bn = self.layer.bn.bn if hasattr(self.layer, "bn") else None
        return dict(w=conv.weight, conv_bias=conv.bias, gamma=bn.weight if bn is not None else None,
                    beta=bn.bias if bn is not None else None, mean=bn.running_mean if bn is not None else None,
                    var=bn.running_var if bn is not None else None, eps=float(bn.eps) if bn is not None else 0.0)


class _Recorder:
    def __init__(self):
        self.jobs = []
        self.parent = {}     # id(part) -> (tensor it was concatenated into, offset)
        self.keep = []       # every tensor whose id is a key above stays alive until the plan is resolved

    def add(self, w, b, phys_map, nbo, fmt, kmajor, out):
        src_w, src_b = getattr(w, "_pack_src", None), getattr(b, "_pack_src", None)
        if src_w is None or src_b is None or src_w[0] is not src_b[0]:
            raise RuntimeError("pack plan: a layer was packed from tensors without provenance (fold_conv_bn -> "
                               "_cols / _pad_rows / _zeros_like_bias is the only supported route)")
        self.jobs.append(PackJob(src_w[0], src_w[1], src_b[1], phys_map, nbo, fmt, kmajor, out))
        self.keep.append(out)

    def placed(self, parts, whole):
        off = 0
        for p in parts:
            assert id(p) not in self.parent
            self.parent[id(p)] = (whole, off)
            off += p.numel()
        self.keep.extend(parts)
        self.keep.append(whole)

    def resolve(self):
        for j in self.jobs:
            t, off = j.dst, 0
            while id(t) in self.parent:
                t, o = self.parent[id(t)]
                off += o
            j.dst, j.dst_off = t, off
            assert off % 4 == 0 and off + j.floats <= t.numel()
        self.parent, self.keep = {}, []
        return self.jobs


@contextlib.contextmanager
def recording():
    """``with recording() as rec``: every ``pack_layer`` / ``_cat`` of fused.py inside reports to ``rec``."""
    global _recorder
    saved, _recorder = _recorder, _Recorder()
    try:
        yield _recorder
    finally:
        _recorder = saved


def note_layer(w, b, phys_map, nbo, fmt, kmajor, out):
    if _recorder is not None:
        _recorder.add(w, b, phys_map, nbo, fmt, kmajor, out)


def note_cat(parts, whole):
    if _recorder is not None:
        _recorder.placed(parts, whole)


class _CJob(ctypes.Structure):       # include/pwclo_ops.h: PwcloPackJob
    _fields_ = ([(n, ctypes.c_void_p) for n in ("w", "conv_bias", "gamma", "beta", "mean", "var", "phys_map", "dst")]
                + [("eps", ctypes.c_double)]
                + [(n, ctypes.c_int) for n in ("cout", "cin", "col0", "use_bias", "nbo", "nbi", "fmt", "kmajor", "tile0",
                                               "reserved")])


_HEAD_PARTS = (("w_qt", "b_qt", "conv1d_q_t"), ("w_q", "b_q", "conv1d_q"), ("w_t", "b_t", "conv1d_t"))


def head_aliases(head, module):
    """Whether every tensor a ``FusedPoseHead`` keeps is a view of its ``PoseCalculator``'s parameter (same address)."""
    return all(getattr(head, w).data_ptr() == getattr(module, blk).conv.weight.data_ptr()
               and getattr(head, b).data_ptr() == getattr(module, blk).conv.bias.data_ptr() for w, b, blk in _HEAD_PARTS)


class PackPlan:
    """The jobs of one ``FusedPWCLONet`` + its pose heads (``heads``: [(FusedPoseHead, PoseCalculator, name)], whose
    weights are views of the parameters and need no job, only a check that they still are)."""

    def __init__(self, recorder, net, heads):
        names = {id(m): n for n, m in net.named_modules()}
        self.jobs = recorder.resolve()
        tile0 = 0
        for j in self.jobs:
            j.name = names.get(id(j.layer), "?")
            j.tile0 = tile0
            tile0 += j.tiles
        self.total_tiles = tile0
        self.heads = list(heads)
        for head, module, name in self.heads:
            if not head_aliases(head, module):
                raise RuntimeError("pack plan: the pose head %s keeps a copy of a parameter, not a view" % name)
        self._ptrs = self._table = self._maps = None
        self._map_off = []
        off = 0
        for j in self.jobs:
            self._map_off.append(off)
            off += len(j.phys_map)
        if self.jobs and self.jobs[0].dst.is_cuda:
            self._upload(self._current())

    # ---- sources ------------------------------------------------------------------------------------------------

    def sources(self):
        """[(qualified name, live tensor or None)] of everything the packed copy depends on, in a fixed order."""
        out, seen = [], set()
        for j in self.jobs:
            if id(j.layer) in seen:
                continue
            seen.add(id(j.layer))
            t = j.tensors()
            out += [(j.name + ".conv.weight", t["w"]), (j.name + ".conv.bias", t["conv_bias"]),
                    (j.name + ".bn.bn.weight", t["gamma"]), (j.name + ".bn.bn.bias", t["beta"]),
                    (j.name + ".bn.bn.running_mean", t["mean"]), (j.name + ".bn.bn.running_var", t["var"])]
        for _, module, name in self.heads:
            for _, _, blk in _HEAD_PARTS:
                conv = getattr(module, blk).conv
                out += [("%s.%s.conv.weight" % (name, blk), conv.weight), ("%s.%s.conv.bias" % (name, blk), conv.bias)]
        return out

    def _current(self):
        return tuple(t.data_ptr() if t is not None else 0 for _, t in self.sources())

    def moved(self):
        """Whether any source tensor's storage is no longer the one the device table points at (``param.data = ...``)."""
        return self._ptrs is not None and self._current() != self._ptrs

    def _first_moved(self, ptrs):
        if self._ptrs is None:
            return "the job table (never written)"
        return next(n for (n, _), a, b in zip(self.sources(), ptrs, self._ptrs) if a != b)

    # ---- device table -------------------------------------------------------------------------------------------

    def _upload(self, ptrs):
        dev = self.jobs[0].dst.device
        # The heads read the parameters through views, and captured graphs hold those views' addresses: a swapped head
        # parameter cannot be followed in place.  (PWCLONet.refresh_fused never gets here: moved() -> it packs again.)
        for head, module, name in self.heads:
            if not head_aliases(head, module):
                raise RuntimeError("pack plan: the storage of a parameter of the pose head %s was swapped; its kernels "
                                   "(and every graph captured over them) read the parameters in place, so this cannot be "
                                   "refreshed: pack again (prepare_fused) and capture again" % name)
        for j in self.jobs:
            t = j.tensors()
            for key in ("w", "conv_bias", "gamma", "beta", "mean", "var"):
                x = t[key]
                if x is None:
                    continue
                rows = x.shape[0] if x.dim() else -1
                if (x.dtype != torch.float32 or not x.is_contiguous() or x.device != dev or rows != j.cout
                        or x.numel() != (j.cout * j.cin if key == "w" else j.cout)):
                    raise RuntimeError("pack plan: %s (%s) changed dtype, device, layout or shape since packing: pack "
                                       "again (prepare_fused)" % (j.name, key))
            if (t["var"] is None) != (t["gamma"] is None) or (t["var"] is None) != (t["mean"] is None) \
                    or (t["var"] is None) != (t["beta"] is None):
                raise RuntimeError("pack plan: %s has a BatchNorm without affine parameters or statistics" % j.name)
            if j.dst.dtype != torch.float32 or j.dst.data_ptr() % 16:
                raise RuntimeError("pack plan: packed buffer of %s is not 16-byte aligned fp32" % j.name)
        if self._maps is None:
            self._maps = torch.tensor([c for j in self.jobs for c in j.phys_map], dtype=torch.int32).to(dev)
            self._table = torch.empty((len(self.jobs) * ctypes.sizeof(_CJob),), dtype=torch.uint8, device=dev)
        p = lambda x: x.data_ptr() if x is not None else None
        table = (_CJob * len(self.jobs))()
        for c, j, moff in zip(table, self.jobs, self._map_off):
            t = j.tensors()
            c.w, c.conv_bias, c.gamma, c.beta = p(t["w"]), p(t["conv_bias"]), p(t["gamma"]), p(t["beta"])
            c.mean, c.var, c.eps = p(t["mean"]), p(t["var"]), t["eps"]
            c.phys_map = self._maps.data_ptr() + 4 * moff
            c.dst = j.dst.data_ptr() + 4 * j.dst_off
            c.cout, c.cin, c.col0, c.use_bias = j.cout, j.cin, j.col0, int(j.use_bias)
            c.nbo, c.nbi, c.fmt, c.kmajor, c.tile0, c.reserved = j.nbo, j.nbi, j.fmt, int(j.kmajor), j.tile0, 0
        host = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8)
        self._table.copy_(host)                 # pageable host memory: the copy has read it when this returns
        self._ptrs = ptrs

    def refresh(self):
        """Rewrite every packed layer from the live module tensors: one launch on the current stream (capturable).  The
        device table is written again only when a source tensor's storage moved, which cannot happen while a stream is
        capturing: RuntimeError naming the tensor.  A pose-head parameter whose storage moved raises always: the heads
        have no packed copy to rewrite."""
        if not self.jobs or not self.jobs[0].dst.is_cuda:
            raise RuntimeError("CPU not supported")
        ptrs = self._current()
        if ptrs != self._ptrs:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("refresh: the storage of %s moved since the job table was written; the table cannot "
                                   "be written while a stream is capturing (refresh once outside capture, or pack again)"
                                   % self._first_moved(ptrs))
            self._upload(ptrs)
        _lib.call("pwclo_pack_layers_kernel_wrapper", self._table.device, self._table.data_ptr(), len(self.jobs),
                  self.total_tiles)
