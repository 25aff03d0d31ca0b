"""What the envelope tests of pools and banks share (tests/test_pool_envelope_host.py, tests/test_gpu_pool_envelope.py, the pins in
tests/test_oracle_golden.py and tests/test_oracle_vs_reference.py): members of one launch that differ in everything the two-block matrix-core
shape admits, at the four forms of the network kernels, and feature rows that reach the wrap of the input quantiser.  Pure host arithmetic.

Widths and the kernel form each reaches, read from the code: kws_pool_create / kws_launch_nn pick <16> where block 0's in_cpad is 16 (up to
16 columns) and <64> otherwise; the kernels set quads = (in_c & 3) == 0 && features is 16-byte aligned.  kws_create accepts all four on the
stub runtime (21 columns: in_cpad 32 inside 64-byte rows), so no width had to be replaced.

Corner graphs.  nn_fits_mfma (csrc/kws_nn_int8_dev.h) asks b.in_cpad == 32 of the second block, that is 17 .. 32 filters in the first: the
issue's ((1,1,7),(1,1,7)) and ((8,3,7),(4,3,7)) run on kws_nn_kernel, and kws_pool_create refuses them by that rule (the GPU test asserts
the refusal and keeps a single-model comparison of both: OUTSIDE).  Their places in the pools are taken by the nearest graphs inside the
shape, ((17,1,7),(1,1,7)) and ((17,3,7),(4,3,7)).  The 1-label graph loads.

Seeds.  A corner's seed is the first one from 6000 + 1000 width + 100 corner on whose drawn input scale and zero point put both wrap
thresholds inside +-6.5 (wrap_thresholds), so that a spiked row can reach them, and on which the graph's scores take at least DISTINCT_MIN
distinct rows over the 64 spiked rows (as drawn, the one-filter graphs often give one row of scores whatever the input); the table below
is the result of that search, and tests/test_pool_envelope_host.py asserts both properties.

What a spike can reach.  cmvnw standardises a column over a window of 101 rows of the 49 frames padded symmetrically: every frame occurs at
least twice in any window, so a single displaced frame comes out at no more than sqrt((101 - 2) / 2) = 7.036 (Z_BOUND) however far it is
displaced; +-40 on N(0, 1) gives 6.84 .. 6.92.  Frame 24 occurs three times in its own window (5.7): no spike is put there.  A member whose
threshold lies beyond Z_BOUND on one side cannot wrap on that side through any call that standardises (every pool and bank call does):
wrap_sides says which sides a member can reach, and both tests assert the wrap on exactly those -- and that every other threshold is
beyond Z_BOUND, so no member sits unexamined between what the spikes give and the bound."""
import numpy as np

from kws_testlib import QUANT_EDGES, quant_edge_blob, synth_model_blob
from pool_testlib import KWS_NN_WAVES, LABELS, POOL_NONE, WIDTHS

WIDTHS4 = {"49x13": WIDTHS["49x13"], "49x16": dict(ncep=16, num_filters=32), "49x21": dict(ncep=21, num_filters=32), "49x40": WIDTHS["49x40"]}
# width -> (CP of kws_pool_nn_mfma_kernel<CP> / kws_bank_nn_mfma*_kernel<CP>, quads with an aligned feature matrix)
KERNEL_FORM = {"49x13": (16, False), "49x16": (16, True), "49x21": (64, False), "49x40": (64, True)}
N_FRAMES = 49
WIN = 101                      # synth_model_blob's cmvnw window
Z_BOUND = float(np.sqrt((WIN - 2) / 2.0))
SPIKE = {"49x13": 40.0, "49x16": 40.0, "49x21": 40.0, "49x40": 40.0}      # the displacement per pool (none had to be raised)
THRESHOLD_MAX = 6.5            # corners: both thresholds inside this

STOCK = ((30, 7, 7), (10, 7, 7))
CORNERS = {
    "max": dict(blocks=((32, 8, 7), (16, 8, 7)), n_labels=48, logit_std=1.5),
    "min": dict(blocks=((17, 1, 7), (1, 1, 7)), n_labels=2),                                     # (the issue's (1,1,7) first block: OUTSIDE)
    "odd": dict(blocks=((17, 2, 7), (5, 5, 7)), n_labels=7, conv_bias=True, add_bias=False),
    "l33": dict(blocks=((32, 1, 7), (1, 8, 7)), n_labels=33),
    "l1": dict(blocks=((17, 3, 7), (4, 3, 7)), n_labels=1),                                      # (the issue's (8,3,7) first block: OUTSIDE)
    "stock": dict(blocks=STOCK, n_labels=4, logit_std=1.5),
}
OUTSIDE = {
    "out_min": dict(blocks=((1, 1, 7), (1, 1, 7)), n_labels=2),
    "out_l1": dict(blocks=((8, 3, 7), (4, 3, 7)), n_labels=1),
}
_SEEDS = {
    "49x13": dict(max=6003, min=6102, odd=6200, l33=6300, l1=6400, stock=6501, out_min=6614, out_l1=6700),
    "49x16": dict(max=7000, min=7101, odd=7202, l33=7300, l1=7400, stock=7502, out_min=7601, out_l1=7701),
    "49x21": dict(max=8000, min=8101, odd=8200, l33=8301, l1=8401, stock=8500, out_min=8603, out_l1=8700),
    "49x40": dict(max=9000, min=9100, odd=9201, l33=9301, l1=9400, stock=9501, out_min=9605, out_l1=9700),
}
# distinct score rows a corner must give over the 64 spiked rows (a graph whose scores never move tests only where they are written): one
# filter in the second block leaves a handful of values, and a single label's softmax is the constant 1 by definition
DISTINCT_MIN = dict(max=32, min=2, odd=32, l33=8, l1=1, stock=32, out_min=2, out_l1=1)
EDGE_PREFIX = {"49x13": "g2/", "49x40": "g2w/"}
N_TENANTS = 3


def in_mfma_shape(blocks):
    """nn_fits_mfma's conditions on the channel and tap counts of a two-block (filters, taps, 7) graph behind 49 frames"""
    (c1, t1, p1), (c2, t2, p2) = blocks
    return 17 <= c1 <= 32 and c2 <= 16 and t1 <= 8 and t2 <= 8 and p1 == 7 and p2 == 7


def corner_kw(width, name):
    """synth_model_blob arguments of a corner (CORNERS or OUTSIDE) at a width"""
    return dict(seed=_SEEDS[width][name], **WIDTHS4[width], **dict(CORNERS, **OUTSIDE)[name])


def tenant_kw4(width, k):
    """pool_testlib.tenant_kw over the four widths: the same tenants at the two widths it knows, seeds of their own at the new ones"""
    base = {"49x13": 4200, "49x40": 5200, "49x16": 6200, "49x21": 7200}[width]
    return dict(seed=base + k, n_labels=LABELS[k % len(LABELS)], logit_std=1.5, **WIDTHS4[width])


def edge_keys(width):
    """the QUANT_EDGES models that share the width's DSP block: 74 at 49x13, 17 at 49x40, none at the new widths"""
    p = EDGE_PREFIX.get(width)
    return [k for k in sorted(QUANT_EDGES) if p and k.startswith(p)]


def member_names(width):
    """the mixed pool of a width, in pool order: the corners, the edge models, tenants 0 .. 2"""
    return list(CORNERS) + edge_keys(width) + ["tenant%d" % k for k in range(N_TENANTS)]


def member_blob(width, name):
    if name in CORNERS or name in OUTSIDE:
        return synth_model_blob(**corner_kw(width, name))
    if name.startswith("tenant"):
        return synth_model_blob(**tenant_kw4(width, int(name[6:])))
    return quant_edge_blob(name)


def write_members(directory, width, names):
    """the .kwsm files of the named members, written once; their paths"""
    import os
    paths = []
    for n in names:
        p = os.path.join(str(directory), "%s_%s.kwsm" % (width, n.replace("/", "_").replace("+", "p")))
        if not os.path.exists(p):
            with open(p, "wb") as f:
                f.write(member_blob(width, n))
        paths.append(p)
    return paths


def bank_names(width):
    """the 16 members of the width's routed bank: every corner and ten edge models spread over the table, the 48- and 33-label ones among them"""
    keys = edge_keys(width)
    pick = [k for k in keys if k.endswith("labels/48") or k.endswith("labels/33")]
    rest = [k for k in keys if k not in pick]
    pick += rest[::max(1, len(rest) // (10 - len(pick)))][:10 - len(pick)]
    return list(CORNERS) + pick


# ---- the member pattern ----------------------------------------------------------------------------------------------------------------------
def member_pattern(names, item_rows, seed=0):
    """the member of each row (uint32, POOL_NONE: nobody): every member gets KWS_NN_WAVES rows, except that corner "max" gets item_rows + 1 (a
    list of two items), corner "odd" exactly item_rows and corner "min" KWS_NN_WAVES - 1; then a row that names nobody goes in at every
    seventh position, and the named rows fill the others in a seeded shuffle"""
    counts = {n: KWS_NN_WAVES for n in names}
    counts["max"], counts["odd"], counts["min"] = item_rows + 1, item_rows, KWS_NN_WAVES - 1
    named = np.concatenate([np.full(counts[n], k, np.uint32) for k, n in enumerate(names)])
    named = named[np.random.default_rng(2000 + seed).permutation(named.size)]
    out, at = [], 0
    while at < named.size:
        if len(out) % 7 == 6:
            out.append(POOL_NONE)
        else:
            out.append(named[at])
            at += 1
    return np.array(out, np.uint32)


def reversed_members(member, K):
    """the same rows for the pool built over the member list reversed"""
    m = np.asarray(member, np.uint32)
    return np.where(m == POOL_NONE, m, np.uint32(K - 1) - m).astype(np.uint32)


def cepstra_members(K, B, call):
    """member per row of the cepstra-in calls (B <= 64 rows each): every seventh row names nobody, the others walk the members from where
    the previous call stopped -- cepstra_calls(K, B) calls give every member a row"""
    m, k = [], call * (B - B // 7)
    for i in range(B):
        if i % 7 == 6:
            m.append(POOL_NONE)
        else:
            m.append(k % K)
            k += 1
    return np.array(m, np.uint32)


def cepstra_calls(K, B):
    per = B - B // 7
    return (K + per - 1) // per


# ---- spiked cepstra ----------------------------------------------------------------------------------------------------------------------------
def spike_frame(b, c):
    """the displaced frame of column c in matrix b: spread over the frames, never the middle one"""
    f = (7 * c + 3 * b + 1) % N_FRAMES
    return f + 1 if f == N_FRAMES // 2 else f


def spiked_cepstra(B, ncep, displacement, seed=77):
    """[B][49][ncep] float32: N(0, 1) values, one frame per column displaced by +-displacement, the sign alternating by column"""
    m = np.random.default_rng(seed).standard_normal((B, N_FRAMES, ncep)).astype(np.float32)
    for b in range(B):
        for c in range(ncep):
            m[b, spike_frame(b, c), c] += np.float32(displacement if c % 2 == 0 else -displacement)
    return m


# ---- the input quantiser restated in numpy float32 ------------------------------------------------------------------------------------------
def input_quant(blob):
    """(scale, zero point) of a blob's input tensor"""
    import eon_import
    tensors, _, t_in, _, _ = eon_import.parse_blob(blob)
    return float(tensors[t_in]["scale"][0]), int(tensors[t_in]["zero"][0])


def unwrapped(features, scale, zp):
    """round(f / scale) + zp before the cast to int8, as int64: the division and the sum in float32, roundf's halves away from zero"""
    v = np.asarray(features, np.float32) / np.float32(scale)
    t = np.trunc(v)
    r = t + np.where(np.abs(v - t) >= np.float32(0.5), np.sign(v), np.float32(0.0)).astype(np.float32)
    q = (r + np.float32(zp)).astype(np.float32)
    assert (np.abs(q) < 2.0 ** 31).all()
    return q.astype(np.int64)


def wrap(u):
    """static_cast<int8_t> of an int32 on the reference's targets: the low byte"""
    return (np.asarray(u, np.int64) & 0xff).astype(np.uint8).view(np.int8)


def wrap_thresholds(scale, zp):
    """(the least feature value that quantises above 127, the greatest that quantises below -128), to within a rounding step"""
    return (127.5 - zp) * scale, (-128.5 - zp) * scale


def wrap_sides(scale, zp):
    """(above, below): which wraps a standardised value can reach at all -- the threshold lies inside Z_BOUND"""
    hi, lo = wrap_thresholds(scale, zp)
    return hi < Z_BOUND, lo > -Z_BOUND


def wrap_counts(features, scale, zp):
    """per feature row: (values above 127, values below -128) before the cast"""
    u = unwrapped(features, scale, zp)
    u = u.reshape(u.shape[0], -1) if u.ndim > 1 else u[None]
    return (u > 127).sum(axis=1), (u < -128).sum(axis=1)


def assert_rows_wrap(features, scale, zp, what):
    """every row wraps on every side its member can reach; a side it cannot reach lies beyond Z_BOUND (wrap_sides), never in between.
    Returns the number of wrapped elements."""
    above, below = wrap_sides(scale, zp)
    n_hi, n_lo = wrap_counts(features, scale, zp)
    assert not above or (n_hi >= 1).all(), (what, "no value above 127 in rows", np.nonzero(n_hi == 0)[0][:4].tolist())
    assert not below or (n_lo >= 1).all(), (what, "no value below -128 in rows", np.nonzero(n_lo == 0)[0][:4].tolist())
    assert above or (n_hi == 0).all(), what
    assert below or (n_lo == 0).all(), what
    return int(n_hi.sum() + n_lo.sum())


def mixed_quads(features, ncep, scale, zp):
    """4-element groups aligned to the channel quad that hold both a wrapped and an unwrapped value (ncep a multiple of 4)"""
    u = unwrapped(features, scale, zp).reshape(-1, 4)
    w = (u > 127) | (u < -128)
    assert ncep % 4 == 0
    return int((w.any(axis=1) & ~w.all(axis=1)).sum())


# ---- the corners pinned to the reference (tests/golden/pool_envelope_l476.npz, tools/make_golden.py --only-pool-envelope) ------------------------
PINNED_WIDTH = "49x13"
PINNED = list(CORNERS) + list(OUTSIDE)


def envelope_golden():
    """name -> dict(out, fc [24][labels] int8, pooled_sha [24][8] uint8): the reference's own op registrations on the 24 rows of
    kws_testlib.quant_edge_inputs(golden_rows=True) for every corner at 49x13"""
    import os
    from kws_testlib import GOLDEN, quant_edge_golden_rows
    g = np.load(os.path.join(GOLDEN, "pool_envelope_l476.npz"))
    n_rows = len(quant_edge_golden_rows())
    offs = np.cumsum([0] + [int(n) * n_rows for n in g["n_labels"]])
    return {str(k): dict(out=g["out"][offs[i]:offs[i + 1]].reshape(n_rows, -1), fc=g["fc"][offs[i]:offs[i + 1]].reshape(n_rows, -1),
                         pooled_sha=g["pooled_sha"][i]) for i, k in enumerate(g["keys"])}
