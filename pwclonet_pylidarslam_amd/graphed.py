"""HIP-graph replay of an eval-mode PWCLO-Net forward.

One PWCLO-Net forward is several hundred short kernels; launched eagerly from Python the GPU
idles between them (measured: 28 ms of kernels in a 100 ms step).  ``GraphedForward`` captures
one forward on fixed-shape buffers into a hipGraph (``torch.cuda.CUDAGraph``; the C-ABI launchers
allocate nothing and never synchronise, so they are capturable) and replays it per batch.
"""
import torch

from . import _lib


class GraphedForward:
    """``GraphedForward(net)(xyz_f1, xyz_f2) -> pose_params (B,4,7)`` for a ``PWCLONet`` in eval
    mode.  Inputs (B,3,N) fp32 on the net's device; a new graph is captured per input shape.
    The returned tensor is a static buffer that the next call overwrites -- clone to keep it."""

    def __init__(self, net, warmup=2, branch=True):
        assert not net.training, "graph capture is for eval mode (fixed control flow, no dropout)"
        self.net = net
        self.warmup = warmup
        self.branch = branch      # fork/join the fused forward's independent branches inside the graph
        self._graphs = {}
        self._saved_log_mode = None

    def _run(self, s1, s2):
        """The captured call on the static input buffers."""
        return self.net(s1, None, s2, None)

    def _capture(self, *inputs):
        net = self.net
        log_mode = net.log_mode
        if log_mode == "host":          # a D2H copy cannot be captured; keep the values on device
            net.log_mode = "device"
        try:
            static = [t.clone() for t in inputs]
            dev = static[0].device
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side), torch.no_grad():
                for _ in range(self.warmup):   # allocator warm-up + one-time kernel attributes
                    self._run(*static)
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize(dev)
            fused = getattr(net, "_fused", None)
            saved_branch = fused.branch if fused is not None else None
            if fused is not None:
                fused.branch = fused.branch and self.branch
            graph = torch.cuda.CUDAGraph()
            try:
                with _lib.capture(graph), torch.no_grad():
                    pose, log = self._run(*static)
            finally:
                if fused is not None:
                    fused.branch = saved_branch
        finally:
            net.log_mode = log_mode
        return graph, static, pose, log

    def _replay(self, *inputs):
        """Copy the inputs into the static buffers of the graph captured for their shapes (captured now if new), replay."""
        key = (tuple(tuple(t.shape) for t in inputs), inputs[0].device)
        if key not in self._graphs:
            self._graphs[key] = self._capture(*inputs)
        graph, static, pose, log = self._graphs[key]
        for dst, src in zip(static, inputs):
            dst.copy_(src)
        graph.replay()
        self.last_log_dict = self._replay_log(log, inputs[0].device)
        return pose

    def __call__(self, xyz_f1, xyz_f2):
        return self._replay(xyz_f1, xyz_f2)

    def _replay_log(self, log, device):
        """log_dict of THIS replay: a fresh lazy view of the graph's static buffers (nothing cached from an
        earlier batch) that waits for the replay before its first read and honours the net's log_mode
        (``host`` -> host tensors, like the reference's log_dict)."""
        if not hasattr(log, "fresh"):
            return log
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(device))
        return log.fresh(to_host=self.net.log_mode == "host", ready=ev.synchronize)


class GraphedSequence(GraphedForward):
    """``GraphedSequence(net, num_points=None)(frames) -> pose_params (T-1, 4, 7)``: ``net.forward_sequence`` on one
    window of T frames (T, n_total, c) replayed from a graph, one per window shape; static output as above."""

    def __init__(self, net, num_points=None, warmup=2, branch=True):
        super().__init__(net, warmup=warmup, branch=branch)
        self.num_points = num_points

    def _run(self, frames):
        return self.net.forward_sequence(frames, self.num_points)

    def __call__(self, frames):
        return self._replay(frames)


class PipelinedForward:
    """Keeps `depth` forwards in flight: one captured graph per slot, used round-robin, on the streams of the native
    stream set (one per slot where the set's probe finds them all running side by side, see ``_submit``; ``describe()``
    says which layout and how many lanes a run got).

    Within one forward the furthest-point-sampling chain is a long dependent sequence that
    occupies one CU per cloud (64 of 256 CUs at batch 32) while the rest of the chip waits; with
    two batches in flight one batch's FPS runs under the other's neighbour-search / MLP kernels.
    Throughput tool: each call returns the (static) output tensor of the slot it used, valid once
    that slot's stream has been synchronised (``wait(slot)`` / ``wait_all()``)."""

    def __init__(self, net, depth=2, streams=None):
        # single-branch graphs: two multi-branch graphs in flight serialise on this runtime
        # (measured: 5.35 ms/step with branches vs 4.0 ms without, 2 in flight)
        import os
        branch = os.environ.get("PWCLO_PIPE_BRANCH", "0") != "0"
        self.slots = [self._make_slot(net, branch) for _ in range(depth)]
        # `streams`: reuse another pipeline's streams -- the runtime binds every new stream to the next
        # hardware queue round-robin, so a second set of streams in one process can collide with itself
        self.streams = list(streams) if streams is not None else None
        assert self.streams is None or len(self.streams) == depth
        # without `streams`: the native library's stream set (pipe_streams.StreamSet: made and first used back to back), or
        # torch's pool streams with PWCLO_PIPE_STREAMS=torch; either is made at the first call, when the device is known
        self._set = None
        self.events = [None] * depth
        self._where = [None] * depth      # the stream each slot's last replay went to
        self._lanes = None                # how many of the streams the calls rotate over (pipe_streams.rotation) ...
        self._order = None                # ... and which: call c goes to streams[_order[c % _lanes]]
        self._next = 0
        self._calls = 0

    def _make_slot(self, net, branch):
        return GraphedForward(net, branch=branch)

    def _make_streams(self, dev):
        from . import pipe_streams
        if pipe_streams.mode() == "torch":
            return [torch.cuda.Stream(device=dev) for _ in self.slots]
        n = min(len(self.slots), pipe_streams.MAX_STREAMS)   # deeper pipelines share streams round-robin
        self._set = pipe_streams.StreamSet(n, dev)
        wrapped = [self._set.wrap(i) for i in range(n)]
        return [wrapped[i % n] for i in range(len(self.slots))]

    def _submit(self, *inputs, after=None):
        """Replay the next slot; ``after(out)``, if given, is queued behind the replay on the same stream.

        Call c uses slot c % depth and stream order[c % lanes].  With lanes == depth that is one stream per slot.  With
        fewer lanes (the native set's probe found fewer streams running side by side than there are slots:
        ``pipe_streams.rotation``; or, in a process that chose no layout, no more hardware queues than slots:
        ``pipe_streams.lanes``) the slots rotate over the streams the probe saw together -- as many replays in flight
        as run side by side, instead of `depth` of which two share a hardware queue -- and a slot's replay first waits for
        the slot's previous one, which ran on another stream."""
        dev = inputs[0].device
        if self.streams is None:
            self.streams = self._make_streams(dev)
        if self._lanes is None:
            self._lanes, self._order = self._rotation()
        i = self._next
        self._next = (i + 1) % len(self.slots)
        st, own = self.streams[self._order[self._calls % self._lanes]], self._set
        self._calls += 1
        # inputs produced on the caller's stream
        if own is not None:
            own.wait_stream(st._pwclo_index, torch.cuda.current_stream(dev))
        else:
            st.wait_stream(torch.cuda.current_stream(dev))
        if self._where[i] is not None and self._where[i] is not st:
            self._stream_wait_slot(st, i)
        with torch.cuda.stream(st):
            out = self.slots[i](*inputs)
            if after is not None:
                after(out)
            if own is not None and i < own.max_slots:
                ev = own.record(i, st._pwclo_index)
            else:                       # torch's pool streams, someone else's streams, or more slots than the set has events for
                ev = torch.cuda.Event()
                ev.record(st)
        self.events[i], self._where[i] = ev, st
        return out, i

    def _probed_set(self):
        """The native set behind ``self.streams`` (this pipeline's own, or the one whose wrappers were passed in)."""
        sets = {id(getattr(s, "_pwclo_set", None)) for s in self.streams}
        return getattr(self.streams[0], "_pwclo_set", None) if len(sets) == 1 else None

    def _rotation(self):
        """(lanes, indices into ``self.streams``): what the set's probe measured (``pipe_streams.rotation``) where the
        process chose a layout; the first ``pipe_streams.lanes(depth)`` streams of a set made for a process that chose
        none; one stream per slot for streams that are not a native set's."""
        from . import pipe_streams
        s = self._probed_set()
        if s is None:
            return len(self.slots), tuple(range(len(self.slots)))
        if not s.follows_probe:
            n = pipe_streams.lanes(len(self.slots))
            return n, tuple(range(n))
        return pipe_streams.rotation(len(self.slots), s.side_by_side, s.together)

    def describe(self):
        """What labels a run: the kind of streams, the set's layout and probe result, the lanes in use (None before the
        first call) and, for comparison, what the queue-count formula ``pipe_streams.lanes`` would have said."""
        from . import pipe_streams
        s = self._probed_set() if self.streams is not None else None
        return dict(streams="unset" if self.streams is None else "torch" if s is None else "native",
                    layout=s.layout if s is not None else None,
                    side_by_side=s.side_by_side if s is not None else None,
                    together=s.together if s is not None else None,
                    follows_probe=s.follows_probe if s is not None else None,
                    lanes=self._lanes, stream_indices=self._order,
                    formula_lanes=pipe_streams.lanes(len(self.slots)))

    def _stream_wait_slot(self, stream, slot):
        """``stream`` waits for the last replay of ``slot`` (and what was queued behind it)."""
        ev = self.events[slot]
        if isinstance(ev, torch.cuda.Event):
            stream.wait_event(ev)
        elif ev is not None:
            self._set.wait_slot(slot, stream)

    def __call__(self, xyz_f1, xyz_f2):
        return self._submit(xyz_f1, xyz_f2)

    def prepare(self, xyz_f1, xyz_f2):
        """Capture every slot's graph now (otherwise a slot is captured on its first use)."""
        for _ in self.slots:
            self(xyz_f1, xyz_f2)
        self.wait_all()

    def wait(self, slot):
        if self.events[slot] is not None:
            self.events[slot].synchronize()

    def wait_all(self):
        if self._set is not None:
            self._set.synchronize()
        else:
            for s in self.streams or []:
                s.synchronize()


def sequence_windows(n, window):
    """How ``PipelinedSequence`` covers an n-frame sequence with windows of ``window`` frames: [(start, length, first)].
    Consecutive windows share their boundary frame; the last one is moved back to end at frame n - 1 and keeps the full
    length (it then overlaps its predecessor by more than one frame), and ``first`` is the first of its pair rows that
    no earlier window produced (0 for all others).  So every pair (i, i + 1) is taken from exactly one window, and every
    window runs P = window - 1 pairs: the pair stage's kernel variants are chosen by the launch size (DESIGN.md section
    10), so a short tail would not give the rows a full window gives.  A sequence shorter than a window is one window."""
    if window < 2:
        raise ValueError("sequence window must hold at least 2 frames (got %d)" % window)
    if n < 2:
        raise ValueError("a sequence needs at least 2 frames (got %d)" % n)
    if n <= window:
        return [(0, n, 0)]
    step = window - 1
    wins = [(s, window, 0) for s in range(0, n - window + 1, step)]
    end = wins[-1][0] + window
    if end < n:
        wins.append((n - window, window, end - 1 - (n - window)))
    return wins


class PipelinedSequence(PipelinedForward):
    """Poses of a long device sequence: ``PipelinedSequence(net, window=33, depth=4)(frames) -> rows (n-1, 4, 7)``,
    frames (n, n_total, c) point-major on the net's device, row i = pair (frame i, frame i + 1) as
    ``net.forward_sequence`` computes it.

    The sequence is cut into windows of ``window`` frames that overlap by one frame (``sequence_windows``; the tail window
    is moved back so that it is full-length too); each window is one replay of a captured ``forward_sequence``
    (``GraphedSequence``), slots used round-robin on their own streams as in ``PipelinedForward``.  Windows share no
    state (the overlap frame's pyramid runs in both), so slots pipeline freely.  Rows are bit-identical to
    ``net.forward_sequence`` on each window; on the whole sequence wherever the pair stage picks the same kernel
    variants for window - 1 and n - 1 pairs.  Each window's new rows are copied into the returned
    tensor on the slot's stream behind the replay; the caller's stream waits for them, so the result is ready in stream
    order and no host sync is made.  A sequence shorter than a window is captured once per length by its slot.  The
    net's ``log_mode`` does not matter here (rows only)."""

    def __init__(self, net, window=33, depth=4, num_points=None, streams=None):
        if window < 2:
            raise ValueError("sequence window must hold at least 2 frames (got %d)" % window)
        self.window, self.num_points = int(window), num_points
        super().__init__(net, depth=depth, streams=streams)

    def _make_slot(self, net, branch):
        return GraphedSequence(net, num_points=self.num_points, branch=branch)

    def __call__(self, frames):
        if not frames.is_cuda:
            raise RuntimeError("CPU not supported")
        n = frames.shape[0]
        wins = sequence_windows(n, self.window)
        rows = torch.empty((n - 1, 4, 7), dtype=torch.float32, device=frames.device)
        used = set()
        for start, length, first in wins:
            dst = rows[start + first:start + length - 1]
            copy = (lambda out, dst=dst, first=first: dst.copy_(out[first:]))
            used.add(self._submit(frames[start:start + length], after=copy)[1])
        main = torch.cuda.current_stream(frames.device)
        for i in used:
            self._stream_wait_slot(main, i)
        return rows


class StagedPipeline:
    """Throughput pipeline that never runs two sampling chains at once.

    A forward is captured as TWO graphs per slot: F = ingest + the furthest-point-sampling chain
    (depends on the input coordinates only; 64 workgroups that each pin a whole CU through their
    LDS table, latency-bound, ~2.5 ms at batch 32) and R = everything else (neighbour search, MFMA
    stacks, pose heads).  All F graphs are replayed on ONE stream, in batch order, so the chains of
    successive batches run back to back on the same 64 CUs; the R graphs alternate between two
    other streams and fill the remaining CUs.  With whole-forward graphs (``PipelinedForward``) two
    batches regularly sit in their F phase together (128 CUs pinned, the rest idle) or in their R
    phase together (no sampling in flight); here exactly one chain is in flight at any time.
    F(i) -> R(i) and R(i) -> F(i + slots) (buffer reuse) are event edges.

    ``pipe(xyz_f1, xyz_f2) -> (pose, slot)``: pose is the slot's static output, valid after
    ``wait(slot)``; a slot is reused every `slots` calls."""

    def __init__(self, net, slots=3, warmup=2):
        assert not net.training and getattr(net, "_fused", None) is not None, \
            "StagedPipeline needs an eval-mode net after prepare_fused()"
        self.net, self.nslots, self.warmup = net, slots, warmup
        self._slots = None
        self._i = 0

    def _capture_slot(self, xyz_f1, xyz_f2):
        fused = self.net._fused
        s1, s2 = xyz_f1.clone(), xyz_f2.clone()
        g_f, g_r = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with _lib.capture(g_f), torch.no_grad():
            state = fused.sample(s1, s2)
        with _lib.capture(g_r, pool=g_f.pool()), torch.no_grad():   # same pool: `state` stays live
            pose, inter = fused.rest(state, return_intermediates=True)
        saved = self.net.log_mode
        self.net.log_mode = "device" if saved == "host" else saved      # no D2H inside a pipeline
        try:
            log = self.net._fused_log_dict(inter)
        finally:
            self.net.log_mode = saved
        return dict(s1=s1, s2=s2, g_f=g_f, g_r=g_r, state=state, pose=pose, log=log, ev_f=None, ev_r=None)

    def _setup(self, xyz_f1, xyz_f2):
        dev = xyz_f1.device
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(self.warmup):          # allocator warm-up + one-time kernel attributes
                self.net._fused(xyz_f1, xyz_f2)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self._slots = [self._capture_slot(xyz_f1, xyz_f2) for _ in range(self.nslots)]
        self.stream_f = torch.cuda.Stream(device=dev)
        self.streams_r = [torch.cuda.Stream(device=dev) for _ in range(2)]
        self._shape = (tuple(xyz_f1.shape), dev)

    def __call__(self, xyz_f1, xyz_f2):
        if self._slots is None:
            self._setup(xyz_f1, xyz_f2)
        assert (tuple(xyz_f1.shape), xyz_f1.device) == self._shape, "StagedPipeline is captured for one input shape"
        i = self._i
        self._i += 1
        k = i % self.nslots
        sl = self._slots[k]
        sf, sr = self.stream_f, self.streams_r[i % 2]
        sf.wait_stream(torch.cuda.current_stream(xyz_f1.device))     # inputs produced on the caller's stream
        if sl["ev_r"] is not None:
            sf.wait_event(sl["ev_r"])                                  # the slot's previous batch is done
        with torch.cuda.stream(sf):
            sl["s1"].copy_(xyz_f1)
            sl["s2"].copy_(xyz_f2)
            sl["g_f"].replay()
            sl["ev_f"] = torch.cuda.Event()
            sl["ev_f"].record(sf)
        sr.wait_event(sl["ev_f"])
        with torch.cuda.stream(sr):
            sl["g_r"].replay()
            sl["ev_r"] = torch.cuda.Event()
            sl["ev_r"].record(sr)
        log = sl["log"]
        self.last_log_dict = (log.fresh(to_host=self.net.log_mode == "host", ready=sl["ev_r"].synchronize)
                              if hasattr(log, "fresh") else log)
        return sl["pose"], k

    def prepare(self, xyz_f1, xyz_f2):
        """Capture all slots now (done on first use otherwise)."""
        if self._slots is None:
            self._setup(xyz_f1, xyz_f2)

    def wait(self, slot):
        ev = self._slots[slot]["ev_r"] if self._slots else None
        if ev is not None:
            ev.synchronize()

    def wait_all(self):
        if self._slots:
            self.stream_f.synchronize()
            for s in self.streams_r:
                s.synchronize()
