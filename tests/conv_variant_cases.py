"""Case table of tests/test_gpu_conv_variants.py: one row per launch of a csrc/conv1x1.hip entry point, each naming the
kernel instantiation it is meant to reach on 256 CUs.  Plain data (no torch): tests/test_conv_plan_cpu.py imports it
to prove, through conv1x1_plan_query, that the rows reach every instantiation the dispatch can select.

Forward family (conv1x1_kernel<NBO, STATS, LEAN>): ``want = (nbo, gy, lean, stats)``.  Weight gradient
(conv1x1_wgrad_kernel<RO, RM, XF>): ``want = (ro, rm, ph)`` and the row's ``xf``.  Sizes are the ENTRY POINT's own
arguments: for "dgrad" and "dgrad_sums" (cin, cout) is the layer, whose cin rows the kernel writes.

Pixel counts.  conv_grid() doubles the channel groups while 2 * ceil(tiles / 8) * gy <= CUs, tiles = b * ceil(p / 32):
below 1025 tiles on 256 CUs a layer of <= 128 output channels runs as NBO = 1.  UNSPLIT is the smallest ragged shape
above that: 3 clouds of 10936 pixels = 341 whole tiles + one of 24 pixels each, 1026 tiles.  UNEVEN (513 tiles) leaves
gy = 2, so the second group owns fewer output blocks than NBO.
"""
import collections

UNSPLIT = (3, 10936)
UNEVEN = (1, 16416)
# (cin, cout) of the NBO ladder: cout = 16 n, cin from {6, 35, 67, 192} (three of them leave an input-channel tail)
LADDER = [(6, 16), (35, 32), (67, 48), (192, 64), (6, 80), (35, 96), (67, 112), (192, 128)]
RAGGED = (67, 100)                    # 7 output blocks, the last one partly empty
POOLED_P = {4: 10936, 8: 10936, 16: 10928, 32: 10944}      # s * k with k | p, still 342 tiles per cloud

Case = collections.namedtuple("Case", "entry b cin cout p want opts")


def _case(entry, bp, cin, cout, want, **opts):
    return Case(entry, bp[0], cin, cout, bp[1], tuple(want), opts)


def case_id(c):
    return "-".join([c.entry, "%dx%dto%dx%d" % (c.b, c.cin, c.cout, c.p), "want" + "_".join(str(v) for v in c.want)]
                    + ["%s%s" % (k, v) for k, v in sorted(c.opts.items())])


def _forward_family():
    rows = []
    nbo = lambda c: -(-c // 16)
    # plain forward and input gradient: the ladder, the ragged block count, the uneven split, one layer beyond 128 channels
    for cin, cout in LADDER + [RAGGED]:
        rows.append(_case("forward", UNSPLIT, cin, cout, (nbo(cout), 1, 1, 0)))
        rows.append(_case("dgrad", UNSPLIT, cout, cin, (nbo(cout), 1, 1, 0)))       # the layer with 16 n INPUT channels
    for cin, cout, want in ((35, 80, 3), (67, 200, 7)):
        rows.append(_case("forward", UNEVEN, cin, cout, (want, 2, 1, 0)))
        rows.append(_case("dgrad", UNEVEN, cout, cin, (want, 2, 1, 0)))
    # general epilogue: all eight widths with ReLU on the un-pooled entry point, three without; 1, 3, 8 on the pooled one
    for cin, cout in LADDER + [RAGGED]:
        rows.append(_case("affine", UNSPLIT, cin, cout, (nbo(cout), 1, 0, 0), relu=1))
    for cin, cout in (LADDER[1], LADDER[4], LADDER[7]):
        rows.append(_case("affine", UNSPLIT, cin, cout, (nbo(cout), 1, 0, 0), relu=0))
    rows.append(_case("affine", UNEVEN, 35, 80, (3, 2, 0, 0), relu=1))
    for k in (4, 8, 16, 32):
        for cin, cout in (LADDER[0], LADDER[2], LADDER[7]):
            rows.append(_case("pooled", (UNSPLIT[0], POOLED_P[k]), cin, cout, (nbo(cout), 1, 0, 0), k=k, relu=1))
    # batch statistics of the output, without and with the on-load BatchNorm + ReLU of the input
    for transform in (0, 1):
        for cin, cout in LADDER:
            rows.append(_case("stats", UNSPLIT, cin, cout, (nbo(cout), 1, 1, 1), transform=transform))
    rows.append(_case("stats", UNEVEN, 35, 80, (3, 2, 1, 1), transform=0))
    # few values per channel on the split path, channel means of 5 standard deviations
    rows.append(_case("stats", (1, 64), 67, 64, (1, 4, 1, 1), transform=0, mean_sigmas=5))
    # BatchNorm-backward sums in the input gradient's epilogue: 1..4 blocks, a ragged third block, the refused fifth
    for affine in (1, 0):
        for cin, cout in ((16, 35), (32, 67), (48, 192), (64, 6)):
            rows.append(_case("dgrad_sums", UNSPLIT, cin, cout, (cin // 16, 1, 1, 2), affine=affine))
    rows.append(_case("dgrad_sums", UNSPLIT, 35, 67, (3, 1, 1, 2), affine=1))
    rows.append(_case("dgrad_sums", UNSPLIT, 80, 35, (5, 1, 1, 2), affine=1, refused=1))
    return rows


# (cin, cout) per (ro, rm, ph): the smallest pairs with a channel tail on both sides that wgrad_plan() gives that form
WGRAD_SHAPES = [((1, 1, 8), 6, 8), ((1, 1, 4), 6, 24), ((1, 1, 2), 3, 35), ((1, 1, 1), 19, 35), ((1, 2, 1), 131, 5),
                ((1, 3, 1), 35, 67), ((1, 4, 1), 387, 3), ((2, 1, 1), 35, 35), ((2, 2, 1), 51, 67), ((2, 3, 1), 67, 67),
                ((2, 4, 1), 387, 19), ((4, 1, 1), 3, 259), ((4, 2, 1), 99, 67), ((4, 3, 1), 67, 131),
                ((4, 4, 1), 99, 131)]
WGRAD_BP = (2, 260)                   # 260 = 8 x 32 + 4 = 2 x 128 + 4: a short last chunk for every cp <= 256


def _wgrad():
    rows = []
    for xf in (0, 1):
        for want, cin, cout in WGRAD_SHAPES:
            opts = dict(xf=xf)
            if want == (1, 1, 8):
                opts["chunk"] = "below"               # p < cp: the only chunk of a row is short
            if want == (1, 1, 1):
                opts["chunk"] = "short"               # several chunks per row, the last one shorter than cp
            rows.append(_case("wgrad", WGRAD_BP, cin, cout, want, **opts))
        # more chunks than workgroups: each walks several (and the row ends in a short one)
        rows.append(_case("wgrad", UNSPLIT, 192, 128, (4, 3, 1), xf=xf, chunk="walk"))
    return rows


CASES = _forward_family() + _wgrad()

# what csrc/conv1x1.hip instantiates: PWCLO_CONV_LAUNCH (28 forms) and PWCLO_WGRAD_LAUNCH (12 rectangles x XF)
INSTANTIATED_FORWARD = ({(n, 0, 1) for n in range(1, 9)} | {(n, 0, 0) for n in range(1, 9)}
                        | {(n, 1, 1) for n in range(1, 9)} | {(n, 2, 1) for n in range(1, 5)})
INSTANTIATED_WGRAD = {(ro, rm, xf) for ro in (1, 2, 4) for rm in (1, 2, 3, 4) for xf in (0, 1)}
