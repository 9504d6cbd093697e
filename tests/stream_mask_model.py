"""Pure-Python model of the per-stream state machine of ``stream_append_masked_kernel``, and the
schedule the CPU and GPU tests run it over.  Per stream and call: idle (not active: nothing but valid = 0), prime
(active and (restart or no previous frame): count = 1, have_prev = 1, valid = 0), pair (otherwise: count + 1, valid = 1;
a full trajectory writes nothing and raises the overflow flag)."""

IDLE, PRIME, PAIR = "idle", "prime", "pair"

# (active, restart) per call for S = 4 streams.  It contains: idle before the first frame (streams 1-3 at call 0), a
# first frame (every stream), pairs, a gap (stream 1 at calls 2-3), a restart while idle (stream 1 at call 3: ignored),
# a restart with a frame (stream 2 at call 4), two streams restarting in the same call (0 and 3 at call 5), idling
# right after a restart (stream 0 at call 6).
SCHEDULE = [
    ((1, 0, 0, 0), (0, 0, 0, 0)),
    ((1, 1, 0, 0), (0, 0, 0, 0)),
    ((1, 0, 1, 1), (0, 0, 0, 0)),
    ((1, 0, 1, 1), (0, 1, 0, 0)),
    ((1, 1, 1, 1), (0, 0, 1, 0)),
    ((1, 1, 1, 1), (1, 0, 0, 1)),
    ((0, 1, 1, 1), (0, 0, 0, 0)),
    ((1, 1, 1, 1), (0, 0, 0, 0)),
]


class StreamMaskModel:
    def __init__(self, streams, capacity):
        self.S, self.capacity = int(streams), int(capacity)
        self.have_prev = [0] * self.S
        self.count = [0] * self.S
        self.valid = [0] * self.S
        self.overflow = 0
        self.calls = 0
        self.last = [None] * self.S       # the call in which each stream delivered its previous frame

    def step(self, active, restart):
        """-> per stream (kind, row, previous call): ``row`` = the trajectory row written (0 for prime, k for pair, None
        when nothing is written), ``previous call`` = the call whose frame a pair is formed with."""
        assert len(active) == len(restart) == self.S
        out = []
        for s in range(self.S):
            if not active[s]:
                self.valid[s] = 0
                out.append((IDLE, None, None))
                continue
            if restart[s] or not self.have_prev[s]:
                self.count[s], self.have_prev[s], self.valid[s] = 1, 1, 0
                out.append((PRIME, 0, None))
            else:
                k = self.count[s]
                if k >= self.capacity:
                    self.overflow = 1
                    row = None
                else:
                    self.count[s] = k + 1
                    row = k
                self.valid[s] = 1
                out.append((PAIR, row, self.last[s]))
            self.last[s] = self.calls
        self.calls += 1
        return out
