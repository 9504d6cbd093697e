"""The (S,) stream masks of per-stream calls (DESIGN.md sections 18 and 21): what ``StreamingOdometry`` and
``registration.IcpRefiner`` share of reading a caller's mask, loading the two words a captured graph reads, and giving
idle streams' rows of a new static input a defined start."""
import numpy as np
import torch


def stream_mask(mask, S, what, owner, indices=False):
    """An (S,) bool or integer mask, host sequence or device tensor -> (S,) int32 0 / 1 tensor where the caller's data
    lives.  ``indices`` (``reset(streams=...)``): integers are stream indices (host sequences only; a device tensor of
    integers is refused as ambiguous), booleans a mask.  Raises ValueError, ``owner`` in front, before anything is
    launched."""
    if isinstance(mask, torch.Tensor) and mask.is_cuda:
        if indices and mask.dtype != torch.bool:
            raise ValueError("%s: reset(%s=...) takes a device mask as bool (integers are stream indices and belong in a "
                             "host list), got %s" % (owner, what, mask.dtype))
        if tuple(mask.shape) != (S,) or mask.dtype.is_floating_point or mask.dtype.is_complex:
            raise ValueError("%s: %s must be a (%d,) bool or integer mask, got %s %s"
                             % (owner, what, S, mask.dtype, tuple(mask.shape)))
        return mask.ne(0).to(torch.int32)
    arr = np.asarray(mask.numpy() if isinstance(mask, torch.Tensor) else mask)
    if indices and arr.ndim == 1 and (arr.dtype.kind in "iu" or arr.size == 0):
        arr = arr.astype(np.int64)
        if arr.size and (arr.min() < 0 or arr.max() >= S):
            raise ValueError("%s: %s %s outside [0, %d)" % (owner, what, arr.tolist(), S))
        out = np.zeros((S,), dtype=np.int32)
        out[arr] = 1
        return torch.from_numpy(out)
    if arr.shape != (S,) or arr.dtype.kind not in "biu":
        raise ValueError("%s: %s must be a (%d,) bool or integer mask, got %s %s" % (owner, what, S, arr.dtype, arr.shape))
    return torch.from_numpy((arr != 0).astype(np.int32))


def load_words(active, restart, act, rst):
    """The call's masks ((S,) int32 0 / 1 tensors anywhere; None: all active, none restarting) into the two device words
    a captured graph reads."""
    if act is None:
        active.fill_(1)
    else:
        active.copy_(act)
    if rst is None:
        restart.zero_()
    else:
        restart.copy_(rst)


def load_lengths(word, lengths, n):
    """The call's ``lengths`` ((S,) int32 anywhere; None: all n rows) into the (S,) device word a captured graph reads."""
    if lengths is None:
        word.fill_(n)
    else:
        word.copy_(lengths)


def seed_idle_rows(act, S, owner, *tensors):
    """New static inputs need every row initialised: idle streams' rows start as copies of the first active stream's.
    ``act``: (S,) int32 mask anywhere (a device mask is read once, here) or None = all active; ``tensors``: (S, ...) or
    None.  -> (host bool mask of the active streams, the tensors: the caller's own where every stream is active, else
    clones with the idle rows filled).  ValueError when no stream is active."""
    host = np.ones((S,), dtype=bool) if act is None else act.cpu().numpy() != 0
    if not host.any():
        raise ValueError("%s: the first call (of an input shape) needs at least one active stream: idle streams' rows "
                         "start as copies of the first active stream's" % owner)
    if host.all():
        return (host,) + tensors
    j, out = int(np.flatnonzero(host)[0]), []
    for t in tensors:
        if t is not None:
            first, t = t[j], t.clone()              # the source row is the caller's: a write may not alias its source
            t[torch.from_numpy(~host).to(t.device)] = first
        out.append(t)
    return (host,) + tuple(out)
