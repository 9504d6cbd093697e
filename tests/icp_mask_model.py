"""Host model of masked (per-stream) point-to-plane registration ("masked registration"), over the
fp64 model of tests/icp_model.py, and the schedule its tests share.  Per stream and call there are two words, ``active``
and ``restart`` (looked at only where active):
  idle     (not active)          the stream's ``Map`` object is not touched; T = init, status IDLE, 0 iterations, 0 pairs
  restart  (active and restart)  the ``Map`` is replaced by an empty one; the frame then finds no live slot, freezes in
                                 iteration 0 with FEW_PAIRS, T = init, and the push fills slot 0
  pair     (otherwise)           ``icp_model.register`` as it is"""
import functools

import numpy as np

import icp_model as model

IDLE = 8

# ---- the schedule: S = 3 streams, M = 2 slots, six calls (numbered from 0) ----------------------------------------------------
S, M, N, CALLS = 3, 2, 1024, 6
ACTIVE = np.array([[1, 1, 0], [1, 0, 1], [1, 1, 1], [0, 1, 1], [1, 1, 1], [1, 1, 1]], dtype=np.int32)
RESTART = np.zeros((CALLS, S), dtype=np.int32)
RESTART[3, 2] = 1                                # stream 2's frame of call 3 starts a new sequence
RESET_BEFORE = {5: [1]}                          # reset(streams=[1]) before call 5


@functools.lru_cache(maxsize=None)
def rooms(n=N):
    """Stream s walks through its own room: (clouds, gt) of ``icp_model.room(3 + s, 6, n)`` per stream."""
    return [model.room(3 + s, CALLS, n) for s in range(S)]


def schedule(n=N):
    """-> list over calls of dict(active (S,), restart (S,), reset: streams to reset before the call, frame (S,): the index
    of the frame stream s delivers (its j-th delivered frame is frame j of its room; -1 when idle), primes (S,) bool: the
    delivered frame only fills the map (first frame, restart, or the first after a reset), cloud (S, n, 3) fp32 (idle
    rows: NaN, nothing may read them), gt (S, 4, 4), init (S, 4, 4): ``perturbed(gt)`` for pairs, I otherwise)."""
    data = rooms(n)
    delivered = [0] * S
    fresh = [True] * S                                            # the next delivered frame finds an empty map
    out = []
    for c in range(CALLS):
        for s in RESET_BEFORE.get(c, []):
            fresh[s] = True
        call = dict(active=ACTIVE[c].copy(), restart=RESTART[c].copy(), reset=RESET_BEFORE.get(c, []),
                    frame=np.full((S,), -1), primes=np.zeros((S,), dtype=bool),
                    cloud=np.full((S, n, 3), np.nan, dtype=np.float32), gt=np.tile(np.eye(4), (S, 1, 1)),
                    init=np.tile(np.eye(4), (S, 1, 1)))
        for s in range(S):
            if not ACTIVE[c, s]:
                continue
            j = delivered[s]
            delivered[s] += 1
            call["frame"][s] = j
            call["cloud"][s] = data[s][0][j]
            call["primes"][s] = fresh[s] or bool(RESTART[c, s])
            fresh[s] = False
            if not call["primes"][s]:
                call["gt"][s] = data[s][1][j]
                call["init"][s] = model.perturbed(data[s][1][j])
        out.append(call)
    return out


class MaskedMaps:
    """S maps under the three-case rule."""

    def __init__(self, streams, M, n, k=10):
        self.maps = [model.Map(M, n, k) for _ in range(streams)]
        self.armed = [False] * streams
        self.M, self.n, self.k = M, n, k

    def reset(self, streams):
        for s in streams:
            self.armed[s] = True

    def register(self, cloud, init, active, restart, **kw):
        """-> list over streams of dict(T, status, iterations, pairs, steps)."""
        out = []
        for s, mp in enumerate(self.maps):
            if not active[s]:
                out.append(dict(T=np.array(init[s], dtype=np.float64), status=IDLE, iterations=0, pairs=0, steps=[]))
                continue
            if restart[s] or self.armed[s]:
                mp = self.maps[s] = model.Map(self.M, self.n, self.k)
                self.armed[s] = False
            T, status, steps = model.register(mp, cloud[s], init[s], **kw)
            moved = [st for i, st in enumerate(steps) if i == 0 or steps[i - 1]["status"] == 0]
            out.append(dict(T=T, status=status, iterations=len(moved), pairs=int(moved[-1]["row"][model.PAIRS]), steps=steps))
        return out
