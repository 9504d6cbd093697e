"""The case table of tests/test_gpu_fps_variants.py, with its clouds, shared with tests/test_fps_plan_cpu.py, which proves
through furthest_point_sampling_plan_query (the code every sampler launcher of csrc/sampling.hip asks) that the rows reach
every form the dispatch can select and sit on both sides of every size boundary.

A case is (entry point, b, n, m, cloud kind, chain arguments, switch set) and the forms it is meant to launch.  A form is a
tag: the kernel instantiation (``fps_reg_kernel<T,E,I,table>``, ``fps_slab_kernel<512,I>``, ``fps_stream_kernel<1024>``), for
the cooperative sampler its order, per-launch regime and launch API (``fps_coop_kernel<16,sorted>/per_launch>=8/cooperative``),
and one tag per chain argument set (``reg+tie_out``, ``reg+prefix_in``, ``reg+both``, ``slab+tie_out``).

Entry points: "auto" = ``_ext.furthest_point_sampling``; "plain" = ``fused.fps_with_xyz`` (the xyz / chain wrappers);
"slab" = ``fused.fps_slab_with_xyz``; "sorted" = the sorted wrapper called directly.

Switch sets: "default"; "capturing" (the stream is under graph capture: plan only); "table0", "coop0", "launch0" = the three
child processes of the GPU test (PWCLO_FPS_TABLE=0; PWCLO_FPS_COOP=0; PWCLO_FPS_COOP_LAUNCH=0 + PWCLO_FPS_COOP_XCD_LOCAL=0 +
PWCLO_FPS_SORTED=0); "order_torch" (PWCLO_FPS_ORDER_TORCH=1: the Python front end's sorts, same kernels: plan only, the
existing test_fps_large_cloud_spatial_orders_agree runs it).

Everything here is CPU torch.  ``python tests/fps_cases.py --child SET`` is the child process of a switch set: it checks the
set's cases against the oracle and prints one JSON line.
"""
import functools
import json
import os
import sys
from collections import namedtuple

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

Case = namedtuple("Case", "name entry b n m cloud chain switches want run")
Case.__new__.__defaults__ = (True,)
Chain = namedtuple("Chain", "tie_out tie_iters prefix_in")
NO_CHAIN = Chain(False, 0, False)

# the rows of fps_reg_kernel and the first / last n of each (tests/test_host_cpu.py derives the same from the source text)
ROW_RANGES = {(64, 0, 1): (1, 64), (64, 0, 2): (65, 127), (64, 1, 1): (128, 128), (64, 1, 2): (129, 255),
              (64, 2, 1): (256, 256), (256, 0, 2): (257, 511), (256, 1, 1): (512, 512), (256, 1, 2): (513, 1024),
              (256, 1, 4): (1025, 2048), (256, 1, 8): (2049, 4096), (512, 0, 16): (4097, 8192),
              (512, 0, 48): (8193, 24576)}
TABLE_LAST_N = 10236                 # 64 + 16 n <= 160 KiB: the last cloud with its copy in LDS (no chain log)
SMALL_CLOUD = 24576                  # the last single-workgroup cloud
SORTED_CLOUD = 32768                 # the first cloud sampled in the spatial order
COOP_POINTS = 16384                  # points of one workgroup of the cooperative sampler
COOP_MAX_G = 32
LARGE_BOUNDARIES = ((SMALL_CLOUD, SMALL_CLOUD + 1), (SORTED_CLOUD - 1, SORTED_CLOUD), (28 * COOP_POINTS, 28 * COOP_POINTS + 1),
                    (COOP_MAX_G * COOP_POINTS, COOP_MAX_G * COOP_POINTS + 1))
SLAB_BOUNDARIES = ((4095, 4096), (8192, 8193), (9216, 9217))

SWITCH_SETS = {      # plan-query arguments of a set; env: what its child process is started with
    "default": dict(args={}, env={}),
    "capturing": dict(args=dict(capturing=True), env=None),
    "order_torch": dict(args=dict(order="torch"), env=None),
    "table0": dict(args=dict(use_table=0), env={"PWCLO_FPS_TABLE": "0"}),
    "coop0": dict(args=dict(use_coop=0), env={"PWCLO_FPS_COOP": "0"}),
    "launch0": dict(args=dict(coop_launch=0, xcd_local=0, use_sorted=0),
                    env={"PWCLO_FPS_COOP_LAUNCH": "0", "PWCLO_FPS_COOP_XCD_LOCAL": "0", "PWCLO_FPS_SORTED": "0"}),
}
CHILD_SETS = ("table0", "coop0", "launch0")


def reg(T, E, I, table):
    return "fps_reg_kernel<%d,%d,%d,%d>" % (T, E, I, table)


def coop(in_order, regime, launch="cooperative"):
    return "fps_coop_kernel<16,%d>/per_launch%s/%s" % (in_order, regime, launch)


STREAM = "fps_stream_kernel<1024>"


def slab(I):
    return "fps_slab_kernel<512,%d>" % I


def row_of(n):
    return next(r for r, (lo, hi) in ROW_RANGES.items() if lo <= n <= hi)


def reg_of(n, chain=None):
    """The reg instantiation of n points under the default switches: the table and the chain log of tie_out fit 160 KiB."""
    log = 8 * (chain.tie_iters + 2) if chain is not None and chain.tie_out else 0
    return reg(*row_of(n), 1 if 64 + 16 * n + log <= 160 * 1024 else 0)


def forms(plan, chain=NO_CHAIN):
    """The tags of a ``_ext.furthest_point_sampling_plan`` answer for a call with these chain arguments."""
    k = plan["kernel"]
    if k == "refused":
        return ("refused",)
    if k == "stream":
        return (STREAM,)
    if k == "coop":
        return (coop(plan["sorted"], ">=8" if plan["per_launch"] >= 8 else "<8", plan["launch"]),)
    if k == "slab":
        return (slab(plan["I"]),) + (("slab+tie_out",) if chain.tie_out else ())
    tags = (reg(plan["T"], plan["E"], plan["I"], plan["table"]),)
    if chain.tie_out or chain.prefix_in:
        tags += ("reg+both" if chain.tie_out and chain.prefix_in else ("reg+tie_out" if chain.tie_out else "reg+prefix_in"),)
    return tags


def plan_of(case, **override):
    from pwclonet_pylidarslam_amd.pointnet2_ops import _ext
    kw = dict(SWITCH_SETS[case.switches]["args"])
    kw.update(override)
    return _ext.furthest_point_sampling_plan(case.b, case.n, case.m, entry=case.entry, tie_iters=case.chain.tie_iters,
                                             tie_out=case.chain.tie_out, prefix_in=case.chain.prefix_in, **kw)


def case_id(c):
    return c.name


# ---- 1. every reg form x cloud kinds: one batch of the five kinds per case ---------------------------------------------------
MIXED = ("uniform", "lattice", "padded0", "few", "none")


def reg_sizes():
    ns = sorted({n for lo_hi in ROW_RANGES.values() for n in lo_hi} | {TABLE_LAST_N, TABLE_LAST_N + 1})
    return ns


def reg_ms(n):
    return sorted({1, 2, min(n, 40), n + 3})


def _reg_cases():
    out = []
    for n in reg_sizes():
        T, E, I = row_of(n)
        out.append(Case("reg-n%d" % n, "auto", len(MIXED), n, n + 3, "mixed", NO_CHAIN, "default",
                        (reg(T, E, I, 1 if n <= TABLE_LAST_N else 0),)))
    return out


REG_CASES = _reg_cases()

# ---- 2. chain forms: (child n = parent m, parent n, parent entry) --------------------------------------------------------------
# one child size per row (the row's last n, and 8193 for the last row: a child of 24576 points has a large-cloud parent,
# which keeps no record); the parents cover ten rows, both slab instantiations and the table flag that the chain log flips
ChainCase = namedtuple("ChainCase", "name parent_entry parent_n child_n")
CHAIN_CASES = [ChainCase("chain-%s-%d-to-%d" % (e, pn, cn), e, pn, cn) for e, pn, cn in (
    ("plain", 127, 64), ("plain", 128, 64), ("plain", 256, 127), ("plain", 512, 128), ("plain", 513, 255), ("plain", 515, 256),
    ("plain", 1025, 511), ("plain", 1027, 512), ("plain", 2051, 1024), ("plain", 4099, 2048), ("plain", 8192, 4096),
    ("plain", 16387, 8192), ("plain", 16389, 8193), ("slab", 8192, 2048), ("slab", 9216, 2048))]
CHAIN_KINDS = ("tiefree", "one_tie", "many_ties")       # one parent batch; "last_tie" has a parent call of its own
LAST_TIE_ITERS = 6                                       # four beacons, then the tie at decision 5 = tie_iters - 1
MANY_TIES_PAIRS = 10                                     # events at decisions 1, 3, ..., 19


def chain_tie_iters(child_n):
    return max(child_n // 2, 2 * MANY_TIES_PAIRS + 4)    # the pyramid's choice, and room for more than eight events


def _chain_plan_cases():
    out = []
    for c in CHAIN_CASES:
        t = chain_tie_iters(c.child_n)
        for tag, ti in (("", t), ("-last", LAST_TIE_ITERS)):
            b = len(CHAIN_KINDS) if not tag else 2
            if c.parent_entry == "slab":
                want = (slab(16 if c.parent_n <= 8192 else 18), "slab+tie_out")
            else:
                want = (reg_of(c.parent_n, Chain(True, ti, False)), "reg+tie_out")
            out.append(Case(c.name + tag + "-parent", c.parent_entry, b, c.parent_n, c.child_n, "chain", Chain(True, ti, False),
                            "default", want))
            for m in sorted({ti, 1}):
                out.append(Case("%s%s-child-m%d" % (c.name, tag, m), "plain", b, c.child_n, m, "chain", Chain(False, 0, True),
                                "default", (reg_of(c.child_n), "reg+prefix_in")))
            both = Chain(True, max(ti - 2, 1), True)
            out.append(Case(c.name + tag + "-child-both", "plain", b, c.child_n, ti, "chain", both, "default",
                            (reg_of(c.child_n, both), "reg+both")))
    # the chain log alone moves the point table out of LDS: 64 + 16 n + 8 (n / 2 + 2) > 160 KiB from n = 8189 on
    out.append(Case("chain-table-flip-8192", "plain", 2, 8192, 4098, "uniform", Chain(True, 4096, False), "default",
                    (reg(512, 0, 16, 0), "reg+tie_out")))
    out.append(Case("chain-table-keep-8188", "plain", 2, 8188, 4096, "uniform", Chain(True, 4094, False), "default",
                    (reg(512, 0, 16, 1), "reg+tie_out")))
    return out


CHAIN_PLAN_CASES = _chain_plan_cases()

# ---- 3. large clouds ------------------------------------------------------------------------------------------------------------
def _large_m(n):
    return 8 if n >= 28 * COOP_POINTS else (32 if n > 100000 else 64)


def _large_cases():
    out = []
    for n, want in ((24577, coop(0, ">=8")), (32767, coop(0, ">=8")), (32768, coop(1, ">=8")), (262144, coop(1, ">=8")),
                    (458752, coop(1, ">=8")), (458753, coop(1, "<8")), (524288, coop(1, "<8")), (524289, STREAM)):
        for cloud in ("padded_100_5000", "lattice"):
            out.append(Case("large-n%d-%s" % (n, cloud), "auto", 1, n, _large_m(n), cloud, NO_CHAIN, "default", (want,)))
    out.append(Case("large-n524289-xyz", "plain", 1, 524289, 8, "padded_100_5000", NO_CHAIN, "default", (STREAM,)))
    out.append(Case("large-n40000-xyz", "plain", 2, 40000, 24, "lattice", NO_CHAIN, "default", (coop(0, ">=8"),)))
    out.append(Case("large-n25000-b9", "auto", 9, 25000, 40, "padded_100_5000", NO_CHAIN, "default", (coop(0, ">=8"),), False))
    return out


LARGE_CASES = _large_cases()

# plan only: the plain-launch forms (a capturing stream; the xyz entry keeps the plain order at every G), not run
PLAN_ONLY_CASES = [
    Case("capture-n24577", "auto", 1, 24577, 8, "uniform", NO_CHAIN, "capturing", (coop(0, ">=8", "plain"),), False),
    Case("capture-n458752", "auto", 1, 458752, 8, "uniform", NO_CHAIN, "capturing", (coop(1, ">=8", "plain"),), False),
    Case("capture-n458753", "auto", 1, 458753, 8, "uniform", NO_CHAIN, "capturing", (coop(1, "<8", "plain"),), False),
    Case("capture-xyz-n524288", "plain", 1, 524288, 8, "uniform", NO_CHAIN, "capturing", (coop(0, "<8", "plain"),), False),
    Case("xyz-n524288", "plain", 1, 524288, 8, "uniform", NO_CHAIN, "default", (coop(0, "<8"),), False),
    Case("sorted-entry-n40000", "sorted", 2, 40000, 8, "uniform", NO_CHAIN, "default", (coop(1, ">=8"),), False),
    Case("order-torch-n40000", "auto", 2, 40000, 96, "uniform", NO_CHAIN, "order_torch", (coop(1, ">=8"),), False),
]

# ---- 4. the spatial order ---------------------------------------------------------------------------------------------------------
ORDER_SIZES = (32768, 32769, 33791)                      # n mod 1024 = 0, 1, 1023
ORDER_KINDS = ("lidar_slab", "planar", "one_eligible", "identical", "none")
ORDER_BATCHES = (("lidar_slab", "planar", "one_eligible", "identical"), ("none", "lidar_slab", "identical", "planar"))

# ---- 5. the slab sampler ----------------------------------------------------------------------------------------------------------
SLAB_KINDS = ("uniform", "lattice", "padded_tail", "wall")
SLAB_CASES = [Case("slab-n%d%s" % (n, "-rec" if rec else ""), "slab", len(SLAB_KINDS), n, 300, "slab",
                   Chain(True, 128, False) if rec else NO_CHAIN, "default",
                   (slab(16 if n <= 8192 else 18),) + (("slab+tie_out",) if rec else ()))
              for n in (4096, 8192, 8193, 9216) for rec in (False, True)]
SLAB_REFUSED = [Case("slab-n%d-refused" % n, "slab", 1, n, 8, "uniform", NO_CHAIN, "default", ("refused",)) for n in (4095, 9217)]

# ---- 6. the switch sets -----------------------------------------------------------------------------------------------------------
SWITCH_CASES = [
    # PWCLO_FPS_TABLE=0: the point table leaves LDS beyond 64 KiB (n = 4092 | 4093)
    Case("table0-n4092", "auto", 5, 4092, 40, "mixed", NO_CHAIN, "table0", (reg(256, 1, 8, 1),)),
    Case("table0-n4093", "auto", 5, 4093, 40, "mixed", NO_CHAIN, "table0", (reg(256, 1, 8, 0),)),
    Case("table0-n4096", "auto", 5, 4096, 40, "mixed", NO_CHAIN, "table0", (reg(256, 1, 8, 0),)),
    Case("table0-n8192", "auto", 5, 8192, 40, "mixed", NO_CHAIN, "table0", (reg(512, 0, 16, 0),)),
    Case("table0-n8193", "auto", 5, 8193, 40, "mixed", NO_CHAIN, "table0", (reg(512, 0, 48, 0),)),
    # PWCLO_FPS_COOP=0: the streaming kernel serves every large cloud
    Case("coop0-n24577-pad", "auto", 1, 24577, 24, "padded_100_5000", NO_CHAIN, "coop0", (STREAM,)),
    Case("coop0-n24577-lattice", "auto", 2, 24577, 24, "lattice", NO_CHAIN, "coop0", (STREAM,)),
    Case("coop0-n40001-pad", "auto", 2, 40001, 24, "padded_100_5000", NO_CHAIN, "coop0", (STREAM,)),
    Case("coop0-n40001-lattice", "auto", 1, 40001, 24, "lattice", NO_CHAIN, "coop0", (STREAM,)),
    Case("coop0-n40001-xyz", "plain", 5, 40001, 24, "mixed", NO_CHAIN, "coop0", (STREAM,)),
    # plain launch, agent-scope exchange, plain order
    Case("launch0-n24577", "auto", 2, 24577, 24, "lattice", NO_CHAIN, "launch0", (coop(0, ">=8", "plain"),)),
    Case("launch0-n40001", "auto", 3, 40001, 24, "padded_100_5000", NO_CHAIN, "launch0", (coop(0, ">=8", "plain"),)),
    Case("launch0-n120000", "auto", 1, 120000, 24, "lattice", NO_CHAIN, "launch0", (coop(0, ">=8", "plain"),)),
]

REFUSED_CASES = [      # (entry, n, plan arguments, a piece of the launcher's message)
    ("auto", 0, {}, "n=0 must be >= 1"), ("plain", 0, {}, "n=0 must be >= 1"),
    ("auto", 1 << 23, {}, "too large"), ("plain", (1 << 23) + 5, {}, "too large"),
    ("plain", 24577, dict(temp=False), "needs the (b,n) temp buffer"),
    ("slab", 4095, {}, "outside the slab sampler's range"), ("slab", 9217, {}, "outside the slab sampler's range"),
    ("slab", 8192, dict(temp=False), "workspace, slab table and status buffer are required"),
    ("sorted", 40000, dict(temp=False), "dataset, sorted copy, permutation and temp are required"),
    ("sorted", 24576, {}, "outside (24576, 2^23)"), ("sorted", 1 << 23, {}, "outside (24576, 2^23)"),
    ("sorted", 524289, {}, "needs 33 workgroups per cloud (max 32)"),
    ("sorted", 40000, dict(temp_aligned=False), "8-byte aligned temp"),
]

ALL_CASES = REG_CASES + CHAIN_PLAN_CASES + LARGE_CASES + PLAN_ONLY_CASES + SLAB_CASES + SWITCH_CASES


@functools.lru_cache(maxsize=None)
def reachable(switches="default"):
    """Every form tag the plan query names for some call the entry points accept under a switch set: all n of the
    single-workgroup range without a record and with the longest record a pyramid asks for (tie_iters = n / 2), both sides of
    the large-cloud boundaries through both entries, capturing or not, and the slab sampler's whole range."""
    from pwclonet_pylidarslam_amd.pointnet2_ops import _ext
    kw = SWITCH_SETS[switches]["args"]
    out = set()
    for n in range(1, SMALL_CLOUD + 1):
        for chain in (NO_CHAIN, Chain(True, n // 2, False), Chain(False, 0, True), Chain(True, n // 2, True)):
            plan = _ext.furthest_point_sampling_plan(2, n, 8, entry="plain", tie_iters=chain.tie_iters, tie_out=chain.tie_out,
                                                     prefix_in=chain.prefix_in, **kw)
            out.update(forms(plan, chain))
    for pair in LARGE_BOUNDARIES + ((120000, 262144),):
        for n in pair:
            for entry in ("auto", "plain"):
                for capturing in (False, True):
                    args = dict(kw, capturing=capturing or kw.get("capturing", False))
                    out.update(forms(_ext.furthest_point_sampling_plan(1, n, 8, entry=entry, **args)))
    for n in range(4096, 9217):
        for chain in (NO_CHAIN, Chain(True, n // 4, False)):
            plan = _ext.furthest_point_sampling_plan(2, n, 8, entry="slab", tie_iters=chain.tie_iters, tie_out=chain.tie_out, **kw)
            out.update(forms(plan, chain))
    out.discard("refused")
    return frozenset(out)


# ---- clouds: (kind, seed, n) -> (n, 3) fp32 -------------------------------------------------------------------------------------
def make_cloud(kind, seed, n):
    gen = torch.Generator().manual_seed(seed * 7919 + n * 31 + sum(map(ord, kind)))
    uni = (torch.rand(n, 3, generator=gen) * 2 - 1) * 20
    if kind == "uniform":
        return uni
    if kind == "lattice":                              # nearly every decision is an exact tie; duplicates
        return torch.randint(-6, 7, (n, 3), generator=gen).float()
    if kind == "padded0":                              # zero padding in front, index 0 included
        uni[:max(1, n // 3)] = 0.0
        return uni
    if kind == "few":                                  # fewer eligible points than samples: exhaustion, repeated indices
        keep = torch.randperm(n, generator=gen)[:min(n, 7)]
        x = torch.full((n, 3), 0.01)                   # |p|^2 = 3e-4 <= 1e-3: never sampled
        x[keep] = uni[keep]
        return x
    if kind == "none":                                 # no eligible point: every index is 0
        return torch.zeros(n, 3)
    if kind == "padded_100_5000":
        uni *= 2
        uni[100:5000] = 0.0
        return uni
    if kind == "padded_tail":
        uni[n - n // 3:] = 0.0
        return uni
    if kind == "wall":                                 # most points share one x: one huge x-bin
        uni[:3 * n // 4, 0] = 3.0
        return uni
    if kind == "lidar_slab":                           # 160 m x 160 m x 4 m, zero padding behind the survivors
        x = (torch.rand(n, 3, generator=gen) * 2 - 1) * torch.tensor([80.0, 80.0, 2.0])
        x[n - n // 5:] = 0.0
        return x
    if kind == "planar":
        uni[:, 2] = 0.0
        return uni
    if kind == "one_eligible":
        x = torch.zeros(n, 3)
        x[(seed * 977 + n // 2) % n] = torch.tensor([1.0, -2.0, 3.0])
        return x
    assert kind == "identical", kind
    return torch.tensor([1.5, -2.25, 7.0]).repeat(n, 1)


def make_batch(case):
    """(b, n, 3) contiguous fp32 on the CPU: "mixed" = the five kinds of MIXED, "slab" = SLAB_KINDS, else b clouds of a kind."""
    kinds = {"mixed": MIXED, "slab": SLAB_KINDS}.get(case.cloud, (case.cloud,) * case.b)
    assert len(kinds) == case.b, case
    return torch.stack([make_cloud(k, 1 + i, case.n) for i, k in enumerate(kinds)]).contiguous()


# chain clouds: a small background cloud around point 0 = (0, 1, 0) and, far outside it, points whose sampling order is fixed by
# construction.  A mirror pair (+-X, 1, Z) is equally far from every sample chosen so far (all of them lie on the plane x = 0
# or come in such pairs): an exact tie, the two points are taken one after the other and the second is alone at its distance
# (2 X is larger): one simple event.  All squared distances stay below the sampler's initial 1e10.
def _background(gen, n):
    x = (torch.rand(n, 3, generator=gen) - 0.5) * 0.8
    x[:, 1] += 1.0
    x[0] = torch.tensor([0.0, 1.0, 0.0])
    return x


def _pairs(x, count, first_slot):
    for j in range(count):                             # the farthest pair is taken first: decisions 1|2, 3|4, ...
        z = 300.0 * (j + 1) + 17.0 * j * j            # uneven spacing: no two pairs are ever equally far from the samples
        x[first_slot + 4 * j] = torch.tensor([5000.0, 1.0, z])
        x[first_slot + 4 * j + 2] = torch.tensor([-5000.0, 1.0, z])


def make_chain_cloud(kind, seed, n):
    assert n >= 100
    gen = torch.Generator().manual_seed(seed * 104729 + n)
    x = _background(gen, n)
    if kind == "tiefree":
        return (torch.rand(n, 3, generator=gen) * 2 - 1) * 20
    if kind == "one_tie":                              # one event, at decision 1
        _pairs(x, 1, 7)
    elif kind == "many_ties":                          # events at decisions 1, 3, ..., 19: more than the record holds
        _pairs(x, MANY_TIES_PAIRS, 5)
    else:                                              # four beacons on the mirror plane (decisions 1..4), then the pair
        assert kind == "last_tie"
        for j in range(4):
            x[11 + 6 * j] = torch.tensor([0.0, 1.0, -400.0 * 2 ** j])
        x[50 + seed], x[90 + seed] = torch.tensor([150.0, 1.0, 100.0]), torch.tensor([-150.0, 1.0, 100.0])
    return x


def make_chain_batch(c, last):
    kinds = ("last_tie", "last_tie") if last else CHAIN_KINDS
    return torch.stack([make_chain_cloud(k, 1 + i, c.parent_n) for i, k in enumerate(kinds)]).contiguous()


# ---- running an entry point -------------------------------------------------------------------------------------------------------
def run(case, x, dev, tie_out=None, prefix_in=None):
    """-> (idx (b, m) int32, new_xyz (b, m, 3) or None) on ``dev`` for the CPU batch x."""
    from pwclonet_pylidarslam_amd import fused
    from pwclonet_pylidarslam_amd.pointnet2_ops import _ext
    xd = x.to(dev)
    if case.entry == "auto":
        return _ext.furthest_point_sampling(xd, case.m), None
    if case.entry == "plain":
        return fused.fps_with_xyz(xd, case.m, tie_out=tie_out, tie_iters=case.chain.tie_iters, prefix_in=prefix_in)
    assert case.entry == "slab"
    idx, new_xyz, _ = fused.fps_slab_with_xyz(xd, case.m, tie_out=tie_out, tie_iters=case.chain.tie_iters)
    return idx, new_xyz


def oracle(x, m):
    from oracle import ops as O
    return O.furthest_point_sampling(x, m)


def gathered(x, idx):
    return torch.gather(x, 1, idx.long().unsqueeze(-1).expand(-1, -1, 3))


def bits(t):
    return t.contiguous().view(torch.int32)


def _child_main(name):
    """Child of test_switch_sets: this process was started with the set's environment."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    spec = SWITCH_SETS[name]
    for k, v in spec["env"].items():
        if os.environ.get(k) != v:
            print(json.dumps({"error": "%s=%s is not set" % (k, v)}))
            return 2
    from pwclonet_pylidarslam_amd import _lib
    dev = torch.device("cuda:0")
    results = {}
    for case in SWITCH_CASES:
        if case.switches != name:
            continue
        plan = plan_of(case)
        # every switch argument left at None: the launchers' own reading of this process's environment
        from pwclonet_pylidarslam_amd.pointnet2_ops import _ext
        env_plan = _ext.furthest_point_sampling_plan(case.b, case.n, case.m, entry=case.entry)
        x = make_batch(case)
        want = oracle(x, case.m)
        idx, new_xyz = run(case, x, dev)
        _lib.synchronize(dev)
        bad = int((idx.cpu() != want).sum())
        if new_xyz is not None:
            bad += int((bits(new_xyz.cpu()) != bits(gathered(x, want))).sum())
        results[case.name] = dict(forms=list(forms(plan)), env_forms=list(forms(env_plan)), xcd_local=env_plan["xcd_local"],
                                  differences=bad)
    print(json.dumps({"set": name, "results": results}))
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child" and sys.argv[2] in CHILD_SETS:
        sys.exit(_child_main(sys.argv[2]))
    sys.exit("usage: fps_cases.py --child {%s}" % "|".join(CHILD_SETS))
