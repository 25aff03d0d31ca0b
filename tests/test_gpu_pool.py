"""Pools on the GPU (kws_pool_*; the contract is in include/kws/kws.h): up to 40 synthetic tenants of the stock two-block int8 graph behind
one DSP block (tests/pool_testlib.py), each row scored by the one member it names.  The score matrix [rows + 2][stride] is filled with the
bit pattern 0x7fc0dead before each call.  A named row must hold, in its member's label columns, the bits of that member's own entry point
in KWS_MODE_EXACT and, on up to 64 rows, match the oracle bit for bit; every other word -- the columns at or above the member's label
count, the rows that name nobody, the two rows past the call -- must still hold the sentinel; `features` must be the single-model call's
bits for every row."""
import sys

import numpy as np
import pytest

from kws_testlib import ROOT, OracleModel, bits, special_clips
from pool_testlib import (KWS_NN_WAVES, PATTERNS, POOL_NONE, SENTINEL_BITS, WIDTHS, check_scores, items_and_rows, load_tenants, pattern,
                          write_tenants)
from scan_testlib import pack, speech

pytestmark = pytest.mark.gpu

CLIP = 16000
K_MAX = 40
SIZES = [1, 9, 203]
ORACLE_ROWS = 64
PAD = 2                        # rows past the call in every output: they must stay the sentinel


@pytest.fixture(scope="module")
def pkg():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def tenants(pkg, oracle, tmp_path_factory):
    """width -> ([loaded model], [oracle model]) of K_MAX tenants, and (width, K) -> the pool over the first K of them; made once"""
    directory = tmp_path_factory.mktemp("pool_tenants")
    made, pools = {}, {}

    def models(width):
        if width not in made:
            paths = write_tenants(directory, width, K_MAX)
            made[width] = (load_tenants(pkg, paths), [OracleModel(oracle, p) for p in paths])
        return made[width]

    def pool(width, K):
        if (width, K) not in pools:
            pools[(width, K)] = pkg.Pool(models(width)[0][:K])
        return pools[(width, K)]

    yield models, pool
    for p in pools.values():
        p.close()
    for gms, _ in made.values():
        for gm in gms:
            gm.close()


@pytest.fixture(scope="module")
def clips(oracle):
    """[203][CLIP] int16: every special clip, then speech-like clips; computed once, never written"""
    sp = np.stack(list(special_clips().values()))
    pcm = np.concatenate([sp, oracle.synth(41, 0, max(SIZES) - sp.shape[0])])
    pcm.setflags(write=False)
    return pcm


@pytest.fixture(scope="module")
def own_rows(tenants, clips):
    """width -> ([scores of each tenant's own run_classifier_batch_device on all clips], tenant 0's features, the clips on the device), once"""
    made = {}

    def get(width):
        import torch
        if width not in made:
            gms = tenants[0](width)[0]
            B = clips.shape[0]
            d = torch.from_numpy(clips.copy()).cuda()
            own = []
            f = torch.empty((B, gms[0].n_features), dtype=torch.float32, device="cuda")
            for k, gm in enumerate(gms):
                s = torch.empty((B, gm.n_labels), dtype=torch.float32, device="cuda")
                gm.run_classifier_batch_device(d.data_ptr(), B, s.data_ptr(), f.data_ptr() if k == 0 else None)
                own.append(s)
            torch.cuda.synchronize()
            made[width] = ([s.cpu().numpy() for s in own], f.cpu().numpy(), d)
        return made[width]

    return get


@pytest.fixture(scope="module")
def oracle_rows(tenants, clips):
    """(width, member, row) -> the oracle's scores of that clip by that tenant; every (member, row) pair is computed once"""
    seen = {}

    def get(width, k, rows):
        missing = [r for r in rows if (width, k, r) not in seen]
        if missing:
            got = tenants[0](width)[1][k].run_batch(clips[missing])
            for r, s in zip(missing, got):
                seen[(width, k, r)] = s
        return np.stack([seen[(width, k, r)] for r in rows])

    return get


def sentinel(rows, cols):
    import torch
    return torch.full((rows, cols), SENTINEL_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def untouched(a):
    return bool((bits(a) == SENTINEL_BITS).all())


def run_batch_case(width, K, B, kind, tenants, own_rows, oracle_rows, with_features):
    pool = tenants[1](width, K)
    own, f_own, d = own_rows(width)
    item_rows = pool.L.kws_pool_item_rows()
    member = pattern(kind, B, K, item_rows, seed=B + K)
    if member is None:
        return False
    stride, F = pool.score_stride, pool.members[0].n_features
    s, f = sentinel(B + PAD, stride), sentinel(B + PAD, F)
    pool.run_classifier_device(d.data_ptr(), B, member, s.data_ptr(), f.data_ptr() if with_features else None)
    s, f = host(s), host(f)
    what = "%s K %d B %d %s" % (width, K, B, kind)
    print(what, "items", len(items_and_rows(member, K, item_rows)[0]))
    check_scores(s, member, own, what)
    assert (same(f[:B], f_own[:B]) and untouched(f[B:])) if with_features else untouched(f), what
    for k in sorted(set(int(m) for m in member[:ORACLE_ROWS] if m != POOL_NONE)):
        rows = [i for i in range(min(B, ORACLE_ROWS)) if member[i] == k]
        assert same(s[rows, :own[k].shape[1]], oracle_rows(width, k, rows)), (what, "oracle", k)
    return True


# ---- clips ---------------------------------------------------------------------------------------------------------------------------
def test_patterns_are_what_they_say():
    """the inputs of the GPU cases, checked as arithmetic: the edge lists sit at the item size's edges for any item size"""
    for item_rows in (4, 16, 64):
        B = 2 * item_rows + KWS_NN_WAVES + 20
        m = pattern("edges", B, 17, item_rows)
        items, rows = items_and_rows(m, 17, item_rows)
        assert [c for k, _, c in items if k == 0] == [item_rows] and [c for k, _, c in items if k == 1] == [item_rows, 1]
        assert [c for k, _, c in items if k == 2] == [KWS_NN_WAVES - 1] and len(items) == 4 and (m == POOL_NONE).sum() == B - len(rows)
        heavy = pattern("heavy", 203, 17, item_rows)
        assert (heavy == 0).sum() == 203 - 16 and all((heavy == k).sum() == 1 for k in range(1, 17))
        assert not (pattern("never", 203, 17, item_rows) == 1).any()


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("K", [1, 17, K_MAX])
def test_pool_clips_match_each_member_and_the_oracle(K, B, tenants, own_rows, oracle_rows):
    """K = 17 is one past a bank; stride 6 with members of 3, 4 and 6 labels (K = 1: stride 3)"""
    pool = tenants[1]("49x13", K)
    assert len(pool) == K and pool.score_stride == (3 if K == 1 else 6)
    ran = [kind for kind in PATTERNS if run_batch_case("49x13", K, B, kind, tenants, own_rows, oracle_rows, with_features=kind != "heavy")]
    assert {"one", "robin", "none", "never"} <= set(ran)
    if B == 203:
        assert "edges" in ran and (K == 1 or "heavy" in ran)


@pytest.mark.parametrize("kind", ["robin", "edges", "none"])
def test_pool_clips_at_64_byte_activation_rows(kind, tenants, own_rows, oracle_rows):
    """the other instantiation of the kernel: 49 x 40 features, kws_pool_nn_mfma_kernel<64>"""
    assert run_batch_case("49x40", 17, 203, kind, tenants, own_rows, oracle_rows, with_features=True)


def test_pool_refuses_a_bad_index_and_writes_nothing(pkg, tenants, own_rows):
    pool = tenants[1]("49x13", 17)
    _, _, d = own_rows("49x13")
    member = pattern("robin", 9, 17, 16)
    member[5] = 17
    member[7] = 4096
    s = sentinel(9, pool.score_stride)
    with pytest.raises(pkg.KwsError) as e:
        pool.run_classifier_device(d.data_ptr(), 9, member, s.data_ptr(), None)
    assert e.value.code == -20 and "clip 5" in str(e.value) and "17" in str(e.value) and untouched(host(s))
    with pytest.raises(pkg.KwsError) as e:
        pool.run_classifier_device(d.data_ptr(), 9, pattern("robin", 9, 17, 16), None, None)
    assert e.value.code == -20
    pool.run_classifier_device(d.data_ptr(), 0, np.zeros(0, np.uint32), s.data_ptr(), None)
    assert untouched(host(s))


@pytest.mark.parametrize("width", list(WIDTHS))
def test_pool_rows_equal_a_routed_bank_of_the_first_sixteen(width, pkg, tenants, own_rows):
    """K = 17, round robin: the rows of members 0 .. 15 are those of a routed bank call over the same sixteen handles with one-hot routes"""
    import torch
    pool = tenants[1](width, 17)
    _, _, d = own_rows(width)
    B = 203
    member = pattern("robin", B, 17, 16)
    s = sentinel(B, pool.score_stride)
    pool.run_classifier_device(d.data_ptr(), B, member, s.data_ptr(), None)
    s = host(s)
    gms = pool.members[:16]
    bank = pkg.Bank(gms)
    try:
        routes = np.where(member < 16, np.uint32(1) << (member % 16), np.uint32(0)).astype(np.uint32)
        out = [sentinel(B, gm.n_labels) for gm in gms]
        bank.run_classifier_routed_device(d.data_ptr(), B, routes, [t.data_ptr() for t in out], None)
        torch.cuda.synchronize()
        for k, gm in enumerate(gms):
            rows = np.nonzero(member == k)[0]
            assert rows.size and same(s[rows, :gm.n_labels], out[k].cpu().numpy()[rows]), (width, k)
    finally:
        bank.close()


# ---- clips of their own lengths ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", list(WIDTHS))
def test_pool_ragged_matches_each_members_own_ragged_call(width, pkg, oracle, tenants):
    """B = 67: 1-frame clips and full clips among lengths in between, at aligned offsets (read in place) and odd ones (staged)"""
    import torch
    K = 17
    pool = tenants[1](width, K)
    gms = pool.members
    B = 67
    rng = np.random.default_rng(67)
    lens = ([640, CLIP, 640 + 319, 9001, CLIP, 5000, 640, 12345] * 9)[:B]
    lens[10:40] = [int(x) for x in rng.integers(640, CLIP + 1, 30)]
    assert lens.count(640) >= 3 and lens.count(CLIP) >= 3 and all(gms[0].window_frame_count(n) >= 1 for n in lens)
    src = oracle.synth(88, 0, B, CLIP)
    buf = np.random.default_rng(9).integers(-32768, 32768, sum(lens) + 16 * B + 64, dtype=np.int16)
    offs, at = [], 0
    for i, n in enumerate(lens):
        at = (at + 7) // 8 * 8 + (i % 2) * (1 + 2 * (i % 4))       # even i: on a 16-byte boundary; odd i: an odd sample
        buf[at:at + n] = src[i][:n]
        offs.append(at)
        at += n
    assert [o % 8 == 0 for o in offs] == [i % 2 == 0 for i in range(B)]
    d = torch.from_numpy(buf).cuda()
    assert d.data_ptr() % 16 == 0
    offs, lens = np.array(offs, np.uint64), np.array(lens, np.uint64)
    member = pattern("none", B, K, 16)
    assert (member == POOL_NONE).any() and all((member == k).any() for k in range(K))
    own, f_own = [], None
    for k, gm in enumerate(gms):
        so, fo = sentinel(B, gm.n_labels), sentinel(B, gm.n_features)
        gm.run_classifier_ragged_device(d.data_ptr(), offs, lens, so.data_ptr(), fo.data_ptr() if k == 0 else None, None)
        own.append(host(so))
        f_own = host(fo) if k == 0 else f_own
    for with_features in (True, False):
        s, f = sentinel(B + PAD, pool.score_stride), sentinel(B + PAD, gms[0].n_features)
        pool.run_classifier_ragged_device(d.data_ptr(), offs, lens, member, s.data_ptr(), f.data_ptr() if with_features else None)
        s, f = host(s), host(f)
        check_scores(s, member, own, (width, "ragged", with_features))
        assert (same(f[:B], f_own) and untouched(f[B:])) if with_features else untouched(f)
    bad = member.copy()
    bad[5] = K
    s = sentinel(B, pool.score_stride)
    with pytest.raises(pkg.KwsError) as e:
        pool.run_classifier_ragged_device(d.data_ptr(), offs, lens, bad, s.data_ptr(), None)
    assert e.value.code == -20 and "clip 5" in str(e.value) and untouched(host(s))


# ---- live continuous streams ---------------------------------------------------------------------------------------------------------
class PoolLive:
    """a pool session next to one single-model session per member, all fed the same pushes: an assigned stream's rows of scores and
    raw_scores in bits against its member's own session, the sentinel everywhere else"""

    def __init__(self, pool, S, sl):
        self.pool, self.gms = pool, pool.members
        self.lv = pool.live_streams(S, sl)
        self.own = [gm.live_streams(S, sl) for gm in self.gms]
        self.assign = np.full(S, POOL_NONE, np.uint32)
        self.counts = set()
        self.rows_checked = 0

    def set(self, streams, member):
        self.lv.assign(streams, member)
        self.assign[list(streams)] = member

    def reset(self, streams):
        self.lv.reset(streams)
        for o in self.own:
            o.reset(streams)

    def push(self, entries, seed):
        import torch
        streams = [e[0] for e in entries]
        chunks = [np.asarray(e[1], np.int16) for e in entries]
        fin = [int(bool(e[2])) for e in entries]
        want = [self.lv.window_count(s, c.size, f) for s, c, f in zip(streams, chunks, fin)]
        self.counts |= set(want)
        n = sum(want)
        pcm, offs, lens = pack(chunks, seed=seed, max_gap=9)
        d = torch.from_numpy(pcm).cuda()
        stride = self.pool.score_stride
        sc, rw = sentinel(n + PAD, stride), sentinel(n + PAD, stride)
        nw = self.lv.push_device(d.data_ptr(), streams, offs, lens, sc.data_ptr(), rw.data_ptr(), finish=fin)
        assert [int(x) for x in nw] == want
        sc, rw = host(sc), host(rw)
        member = np.repeat(self.assign[streams], want).astype(np.uint32) if streams else np.zeros(0, np.uint32)
        so_all, ro_all = [], []
        for k, gm in enumerate(self.gms):
            so, ro = sentinel(max(n, 1), gm.n_labels), sentinel(max(n, 1), gm.n_labels)
            nwo = self.own[k].push_device(d.data_ptr(), streams, offs, lens, so.data_ptr(), ro.data_ptr(), finish=fin)
            assert [int(x) for x in nwo] == want
            so_all.append(host(so)[:n])
            ro_all.append(host(ro)[:n])
        check_scores(sc, member, so_all, ("scores", streams))
        check_scores(rw, member, ro_all, ("raw_scores", streams))
        self.rows_checked += int((member != POOL_NONE).sum())
        return want

    def close(self):
        self.lv.close()
        for o in self.own:
            o.close()


@pytest.mark.parametrize("width", list(WIDTHS))
def test_pool_live_pushes_match_the_members_own_sessions(width, pkg, oracle, tenants):
    """S = 12, K = 5: pushes of no samples, of less than a slice and of several slices; streams that finish; a reset and a new member after
    it; stream 11 stays unassigned -- its windows are counted, its rows stay the sentinel"""
    pool = tenants[1](width, 5)
    S, sl, g = 12, 4000, 320
    recs = [speech(oracle, 1200 + s, 12 * sl + g + 7 + s) for s in range(S)]
    again = speech(oracle, 1250, 7 * sl + g)
    chk = PoolLive(pool, S, sl)
    try:
        chk.set(range(S - 1), [s % 5 for s in range(S - 1)])
        assert chk.assign[S - 1] == POOL_NONE
        pos = [0] * S

        def take(s, n, rec=None):
            rec = recs[s] if rec is None else rec
            c = rec[pos[s]:pos[s] + n]
            pos[s] += c.size
            return c
        chk.push([(s, take(s, 3 * sl), False) for s in range(S)], seed=1)                                    # no window yet
        w = chk.push([(s, take(s, sl + g), False) for s in range(S)], seed=2)                                # the first window of each
        assert w == [1] * S
        # an assigned and an unassigned stream that have been pushed to keep what they have: refused, naming the entry
        for streams, member in (([3, 0], [1, 2]), ([S - 1], [0])):
            with pytest.raises(pkg.KwsError) as e:
                chk.lv.assign(streams, member)
            assert e.value.code == -20 and "entry 0" in str(e.value) and "pushed" in str(e.value)
        w = chk.push([(11, take(11, 3 * sl), False), (4, take(4, 3 * sl), False), (0, take(0, 100), False), (7, take(7, 0), False), (2, take(2, 2 * sl + 5), False)], seed=3)
        assert w == [3, 3, 0, 0, 2]
        w = chk.push([(1, take(1, 17), True), (2, take(2, 0), False), (11, take(11, sl), True)], seed=4)      # two streams finish
        assert w[1] == 0
        # the finished streams are in their start state: stream 11 gets a member, stream 1 another one; stream 3 after a reset too
        chk.set([11, 1], [4, 0])
        chk.reset([3])
        chk.set([3], [POOL_NONE])
        pos[3] = pos[1] = pos[11] = 0
        w = chk.push([(3, take(3, 5 * sl + g, again), False), (11, take(11, 6 * sl + g), False), (1, take(1, 4 * sl + g), False), (0, take(0, sl - 1), False)], seed=5)
        assert w[0] == 2 and w[1] == 3
        chk.push([(s, take(s, recs[s].size), True) for s in (0, 2, 4, 5, 11)], seed=6)
        assert {0, 1, 2, 3} <= chk.counts and chk.rows_checked >= 40
    finally:
        chk.close()


def test_pool_live_push_over_two_chunks_of_the_finishing_step(pkg, tenants):
    """The finishing step takes at most 64 MiB of gathered windows at a time: 8 559 windows of 49 x 40 features.  One push of 12 streams x 714
    windows (8 568) spans two chunks -- the second chunk's member table, row offset and upload -- and is compared, scores and raw scores, with
    a second session fed the same audio in two pushes that fit one chunk each."""
    import torch
    pool = tenants[1]("49x40", 5)
    F = pool.members[0].n_features
    chunk = (64 << 20) // (4 * F)
    S, sl, per = 12, 4000, 714
    assert (S - 1) * per <= chunk < S * per
    n1 = (per + 3) * sl + 320
    d = torch.empty((S, n1), dtype=torch.int16, device="cuda")
    pkg.synth_clips_device(91, 0, S, n1, d.data_ptr())
    streams = list(range(S))
    member = np.array([s % 5 for s in streams], np.uint32)
    member[7] = POOL_NONE
    offs = [s * n1 for s in streams]
    stride = pool.score_stride
    one, two = pool.live_streams(S, sl), pool.live_streams(S, sl)
    try:
        one.assign(streams, member)
        two.assign(streams, member)
        a, ra = sentinel(S * per + PAD, stride), sentinel(S * per + PAD, stride)
        nw = one.push_device(d.data_ptr(), streams, offs, [n1] * S, a.data_ptr(), ra.data_ptr())
        assert [int(x) for x in nw] == [per] * S
        half = 400 * sl
        b1, rb1 = sentinel(S * per, stride), sentinel(S * per, stride)
        b2, rb2 = sentinel(S * per, stride), sentinel(S * per, stride)
        nw1 = two.push_device(d.data_ptr(), streams, offs, [half] * S, b1.data_ptr(), rb1.data_ptr())
        nw2 = two.push_device(d.data_ptr(), streams, [o + half for o in offs], [n1 - half] * S, b2.data_ptr(), rb2.data_ptr())
        w1, w2 = int(nw1[0]), int(nw2[0])
        assert w1 + w2 == per and S * max(w1, w2) <= chunk and all(int(x) == w1 for x in nw1) and all(int(x) == w2 for x in nw2)
        torch.cuda.synchronize()
        ai, rai = a.view(torch.int32), ra.view(torch.int32)
        for s in streams:
            for got, p1, p2 in ((ai, b1, b2), (rai, rb1, rb2)):
                rows = got[s * per:(s + 1) * per]
                want = torch.cat([p1.view(torch.int32)[s * w1:(s + 1) * w1], p2.view(torch.int32)[s * w2:(s + 1) * w2]])
                assert bool((rows == want).all()), s
                labels = 0 if s == 7 else pool.members[int(member[s])].n_labels
                assert bool((rows[:, labels:] == SENTINEL_BITS).all()) and (labels == 0 or bool((rows[:, :labels] != SENTINEL_BITS).all())), s
        assert bool((ai[S * per:] == SENTINEL_BITS).all()) and bool((rai[S * per:] == SENTINEL_BITS).all())
    finally:
        one.close()
        two.close()
