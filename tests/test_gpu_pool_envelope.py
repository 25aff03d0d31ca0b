"""Pools and banks across the two-block envelope and the wrap of the input quantiser, on the GPU (tests/pool_envelope_testlib.py says what the
members, widths and spiked cepstra are; tests/test_pool_envelope_host.py checks those inputs with the restatement).  One launch serves members
that differ in filters, taps, padding, biases and label counts (1 .. 48, score stride 48), at all four forms of the network kernels.  Every
output is filled with the bit pattern 0x7fc0dead before each call, PAD rows past the call included; every comparison is bit for bit against
the restatement (oracle/) or the sentinel -- the one pair of library calls compared with each other is the aligned / unaligned feature
matrix, and both of those are held to the restatement too.  Raw scores of continuous mode, for which the restatement has no output of its
own, are tied to the filtered ones through the moving average restated in numpy (scan_testlib.moving_average)."""
import sys

import numpy as np
import pytest

import pool_envelope_testlib as E
from kws_testlib import ROOT, OracleModel, bits, special_clips
from pool_testlib import POOL_NONE, SENTINEL_BITS
from scan_testlib import moving_average, oracle_scan, pack, speech

pytestmark = pytest.mark.gpu

PAD = 2                        # rows past the call in every output: they must stay the sentinel
B_CEP = 64
TAPS = 2                       # EI_CLASSIFIER_SLICES_PER_MODEL_WINDOW >> 1
UNSUPPORTED = -18              # KWS_ERROR_UNSUPPORTED_MODEL


@pytest.fixture(scope="module")
def pkg():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401
    from __graft_entry__ import load_package
    return load_package()


class Env:
    """a width's members -- the mixed pool's, then the two graphs outside the shape -- loaded once on both sides, and its pools"""

    def __init__(self, pkg, oracle, directory, width):
        self.width, self.names = width, E.member_names(width)
        self.K = len(self.names)
        every = self.names + list(E.OUTSIDE)
        paths = E.write_members(directory, width, every)
        self.gm = {n: pkg.Model(p) for n, p in zip(every, paths)}
        self.om = {n: OracleModel(oracle, p) for n, p in zip(every, paths)}
        self.quant = {n: E.input_quant(open(p, "rb").read()) for n, p in zip(every, paths)}
        for n in every:
            assert not self.gm[n].is_float and (self.gm[n].nn_kernel == "kws_nn_mfma_kernel") == (n not in E.OUTSIDE), (width, n, self.gm[n].nn_kernel)
        self.pool = pkg.Pool([self.gm[n] for n in self.names])
        self.pool_rev = pkg.Pool([self.gm[n] for n in self.names[::-1]])
        self.F = self.gm[self.names[0]].n_features
        self.banks = {}

    def close(self):
        for b in self.banks.values():
            b.close()
        self.pool.close()
        self.pool_rev.close()
        for gm in self.gm.values():
            gm.close()


@pytest.fixture(scope="module")
def envs(pkg, oracle, tmp_path_factory):
    directory = tmp_path_factory.mktemp("pool_envelope")
    made = {}

    def get(width):
        if width not in made:
            made[width] = Env(pkg, oracle, directory, width)
        return made[width]

    yield get
    for e in made.values():
        e.close()


@pytest.fixture(scope="module")
def clips(oracle):
    """[420][16000] int16: every special clip, then speech-like clips; computed once, never written"""
    sp = np.stack(list(special_clips().values()))
    pcm = np.concatenate([sp, oracle.synth(47, 0, 420 - sp.shape[0])])
    pcm.setflags(write=False)
    return pcm


@pytest.fixture(scope="module")
def cepstra(oracle):
    """width -> (the spiked cepstra [B_CEP][49 ncep], their standardised rows by Oracle.cmvnw); computed once, never written"""
    made = {}

    def get(width):
        if width not in made:
            m = E.spiked_cepstra(B_CEP, E.WIDTHS4[width]["ncep"], E.SPIKE[width])
            f = np.stack([oracle.cmvnw(x, E.WIN).reshape(-1) for x in m])
            m = np.ascontiguousarray(m.reshape(B_CEP, -1))
            m.setflags(write=False)
            f.setflags(write=False)
            made[width] = (m, f)
        return made[width]

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


def assert_bits(got, want, what):
    bad = np.argwhere(bits(got) != want)
    assert bad.size == 0, (what, "first differing (row, column):", bad[:4].tolist())


def expected(rows, stride, pairs):
    """[rows][stride] bits: the sentinel, but for pairs (row, scores of its member by the restatement) in the member's label columns"""
    want = np.full((rows, stride), SENTINEL_BITS, np.uint32)
    for r, s in pairs:
        want[r, :s.size] = bits(s)
    return want


# ---- mixed pools from audio ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", list(E.WIDTHS4))
def test_mixed_pool_clips_match_the_restatement_as_built_and_reversed(width, envs, clips):
    """about 4 rows per member (83 members and 400 rows at 49x13), every named row against OracleModel.run_batch of its member, the features
    of every row against the restatement and against member 0's own call; then the pool over the reversed member list -- another graph
    supplies the front end, the activation-row width and the scratch -- on the same rows: the same bits"""
    import torch
    env = envs(width)
    assert len(env.pool) == env.K and env.pool.score_stride == env.pool_rev.score_stride == 48
    item_rows = env.pool.L.kws_pool_item_rows()
    member = E.member_pattern(env.names, item_rows, seed=env.K)
    B = member.size
    assert B <= clips.shape[0]
    d = torch.from_numpy(clips[:B].copy()).cuda()
    pairs, want_f = [], np.zeros((B, env.F), np.float32)
    for k, n in enumerate(env.names):
        at = np.nonzero(member == k)[0]
        s, f, _ = env.om[n].run_batch(clips[at], want_features=True)
        pairs += list(zip(at, s))
        want_f[at] = f
    at = np.nonzero(member == POOL_NONE)[0]
    want_f[at] = env.om[env.names[0]].run_batch(clips[at], want_features=True)[1]
    want = expected(B + PAD, 48, pairs)
    assert len(pairs) == (member != POOL_NONE).sum() >= 4 * env.K - 1
    for pool, m in ((env.pool, member), (env.pool_rev, E.reversed_members(member, env.K))):
        s, f = sentinel(B + PAD, 48), sentinel(B + PAD, env.F)
        pool.run_classifier_device(d.data_ptr(), B, m, s.data_ptr(), f.data_ptr())
        s, f = host(s), host(f)
        what = (width, "reversed" if pool is env.pool_rev else "as built")
        assert_bits(s, want, what)
        assert same(f[:B], want_f) and untouched(f[B:]), what
        f0 = sentinel(B + PAD, env.F)
        s0 = sentinel(B, pool.members[0].n_labels)
        pool.members[0].run_classifier_batch_device(d.data_ptr(), B, s0.data_ptr(), f0.data_ptr())
        assert same(host(f0), f), what
        # without features: the pool's own matrix
        s2 = sentinel(B + PAD, 48)
        pool.run_classifier_device(d.data_ptr(), B, m, s2.data_ptr(), None)
        assert_bits(host(s2), want, what + ("no features",))


# ---- the quantiser's wrap -----------------------------------------------------------------------------------------------------------------
def run_cepstra(env, pool, names, mfcc_d, member, features_ptr=None):
    """one cepstra-in call on the B_CEP spiked rows -> (scores, features) on the host, features written to features_ptr or a fresh matrix"""
    s = sentinel(B_CEP + PAD, 48)
    f = None
    if features_ptr is None:
        f = sentinel(B_CEP + PAD, env.F)
        features_ptr = f.data_ptr()
    pool.cmvn_inference_device(mfcc_d.data_ptr(), B_CEP, member, s.data_ptr(), features_ptr)
    return host(s), None if f is None else host(f)


def check_cepstra(env, names, member, s, f, want_f, what):
    """features against the restatement's cmvnw; each named row's scores against OracleModel.run_inference of the returned features; and
    the rows under test wrapped for their member (E.assert_rows_wrap on the returned features).  Returns the wrapped elements per member."""
    assert same(f[:B_CEP], want_f) and untouched(f[B_CEP:]), what
    pairs, wrapped = [], {}
    for k, n in enumerate(names):
        at = np.nonzero(member == k)[0]
        if at.size:
            pairs += [(r, env.om[n].run_inference(f[r])) for r in at]
            wrapped[n] = E.assert_rows_wrap(f[at], *env.quant[n], what + (n,)) / at.size
    assert_bits(s, expected(B_CEP + PAD, 48, pairs), what)
    return wrapped


@pytest.mark.parametrize("width", list(E.WIDTHS4))
def test_cepstra_in_rows_that_wrap_the_quantiser(width, envs, cepstra):
    """the spiked cepstra through kws_pool_cmvn_inference_device, in as many calls of 64 rows as give every member a row: one value per
    column and row lies beyond the int8 range before the cast (13 of 637, 16 of 784, 21 of 1029, 40 of 1960 for a member that wraps on both
    sides), so the low byte is what reaches the network -- in the quads widths packed into one word with three values that did not wrap"""
    import torch
    env = envs(width)
    m, want_f = cepstra(width)
    mfcc_d = torch.from_numpy(m.copy()).cuda()
    seen, wrapped = set(), {}
    for call in range(E.cepstra_calls(env.K, B_CEP)):
        member = E.cepstra_members(env.K, B_CEP, call)
        s, f = run_cepstra(env, env.pool, env.names, mfcc_d, member)
        wrapped.update(check_cepstra(env, env.names, member, s, f, want_f, (width, call)))
        seen |= set(int(x) for x in member if x != POOL_NONE)
        if call == 0:
            gm0 = env.pool.members[0]
            s0, f0 = sentinel(B_CEP, gm0.n_labels), sentinel(B_CEP + PAD, env.F)
            gm0.cmvn_inference_batch_device(mfcc_d.data_ptr(), B_CEP, s0.data_ptr(), f0.data_ptr())
            assert same(host(f0), f), width
    assert seen == set(range(env.K))
    print(width, "kernel form <%d> %s; wrapped elements per row:" % (E.KERNEL_FORM[width][0], "quads" if E.KERNEL_FORM[width][1] else "scalar"),
          {n: wrapped[n] for n in list(E.CORNERS) + ["tenant0", "tenant1", "tenant2"]})
    assert all(wrapped[n] >= 2 for n in list(E.CORNERS) + ["tenant0", "tenant1"])
    if E.KERNEL_FORM[width][1]:
        assert all(E.mixed_quads(want_f[0], E.WIDTHS4[width]["ncep"], *env.quant[n]) >= 1 for n in E.CORNERS)


@pytest.mark.parametrize("width", ["49x16", "49x40"])
def test_features_off_a_16_byte_boundary_take_the_scalar_loads(width, envs, cepstra):
    """`features` 4 bytes past a 16-byte boundary: the kernels that write it (kws_cmvn_nn_kernel, kws_cmvn_lds_kernel, kws_cmvn_generic_kernel)
    store one float at a time, and the network kernels test the base before they load four (quads = ... && ((uintptr_t)features & 15) == 0),
    so the call is served -- by the scalar path of the quads widths.  Scores and features: the bits of the aligned call and of the restatement;
    the words either side of the matrix keep the sentinel."""
    import torch
    env = envs(width)
    m, want_f = cepstra(width)
    mfcc_d = torch.from_numpy(m.copy()).cuda()
    member = E.cepstra_members(env.K, B_CEP, 0)
    s_al, f_al = run_cepstra(env, env.pool, env.names, mfcc_d, member)
    buf = sentinel(1, (B_CEP + PAD) * env.F + 8)
    assert buf.data_ptr() % 16 == 0
    s_un, _ = run_cepstra(env, env.pool, env.names, mfcc_d, member, features_ptr=buf.data_ptr() + 4)
    flat = host(buf).reshape(-1)
    f_un = flat[1:1 + (B_CEP + PAD) * env.F].reshape(B_CEP + PAD, env.F)
    assert untouched(flat[:1]) and untouched(flat[1 + B_CEP * env.F:])
    assert same(s_un, s_al) and same(f_un, f_al)
    check_cepstra(env, env.names, member, s_un, f_un, want_f, (width, "unaligned"))


# ---- stride 48 in continuous mode ---------------------------------------------------------------------------------------------------------
CONT = ["max", "l33", "l1", "g2/labels/47", "g2/labels/13", None]       # who the recordings and streams go to (None: nobody)


def check_life(env, name, audio, sc, rw, finished, sl, what):
    """one stream from a start to a finish or reset, or one recording: its rows of scores against the restated continuous mode over the audio
    it heard (all windows if it finished, else the first ones), its raw rows tied to them through the moving average; columns at or above
    the member's label count, and every column of a stream that names nobody, still the sentinel"""
    sc, rw = np.asarray(sc, np.float32).reshape(-1, 48), np.asarray(rw, np.float32).reshape(-1, 48)
    if name is None:
        assert untouched(sc) and untouched(rw), what
        return 0
    L = env.om[name].n_labels
    want = oracle_scan(env.om[name], audio, sl)
    assert (want.shape[0] == sc.shape[0]) if finished else (want.shape[0] >= sc.shape[0]), (what, want.shape, sc.shape)
    assert same(sc[:, :L], want[:sc.shape[0]]), what
    assert same(moving_average(rw[:, :L], TAPS), sc[:, :L]), what
    assert untouched(sc[:, L:]) and untouched(rw[:, L:]), what
    return sc.shape[0]


def test_scan_at_stride_48(envs, oracle):
    """recordings of the 48-, 33- and 1-label corners, two label-count edge models and nobody in one scan of the 49x13 mixed pool: 64-thread
    blocks of the moving average straddle entries of 48 columns; two recordings are too short for a window"""
    import torch
    env = envs("49x13")
    gm0, sl, g = env.pool.members[0], 4000, 320
    who = [None, "max", "l33", "g2/labels/47", "l1", "max", "g2/labels/13", None, "l1", "l33"]
    lens = [3 * sl, 2 * sl + 7, 4 * sl + g, 9 * sl + 11, 6 * sl + g - 1, 11 * sl + g, 5 * sl, 7 * sl + g, 4 * sl + g + 1, sl - 1]
    recs = [speech(oracle, 1700 + i, n) for i, n in enumerate(lens)]
    pcm, offs, ln = pack(recs, seed=31, max_gap=9)
    W = [gm0.scan_window_count(int(x), sl) for x in ln]
    assert W[0] == W[1] == W[9] == 0 and min(W[2:9]) >= 1 and max(W) >= 8
    member = np.array([POOL_NONE if n is None else env.names.index(n) for n in who], np.uint32)
    d = torch.from_numpy(pcm).cuda()
    n = sum(W)
    s, r = sentinel(n + PAD, 48), sentinel(n + PAD, 48)
    env.pool.scan_recordings_device(d.data_ptr(), offs, ln, member, s.data_ptr(), r.data_ptr(), slice_samples=sl)
    s, r = host(s), host(r)
    cut = np.cumsum([0] + W)
    checked = sum(check_life(env, who[i], recs[i], s[cut[i]:cut[i + 1]], r[cut[i]:cut[i + 1]], True, sl, ("scan", i)) for i in range(len(who)))
    assert checked == n - W[7] and untouched(s[n:]) and untouched(r[n:])
    # without raw scores: filtered in place, the same bits
    s2 = sentinel(n + PAD, 48)
    env.pool.scan_recordings_device(d.data_ptr(), offs, ln, member, s2.data_ptr(), None, slice_samples=sl)
    assert same(host(s2), s)


def test_live_streams_at_stride_48(envs, oracle):
    """eight streams of the 49x13 mixed pool over seven pushes: the members of CONT, a stream that finishes early, and a stream that is
    reset and goes from the 48-label member to the 1-label one -- columns 1 .. 47 of its later rows, which its filter used before, keep
    the sentinel"""
    import torch
    env = envs("49x13")
    S, sl, g = 8, 4000, 320
    who = list(CONT) + ["l33", "max"]                             # stream 6 finishes early; stream 7 is reset and reassigned
    recs = [speech(oracle, 1800 + s, 8 * sl + g + 5 + s) for s in range(S)]
    again = speech(oracle, 1850, 6 * sl + g)
    lv = env.pool.live_streams(S, sl)
    try:
        lv.assign(range(S), [POOL_NONE if n is None else env.names.index(n) for n in who])
        life = [dict(name=who[s], audio=np.zeros(0, np.int16), sc=[], rw=[], finished=False) for s in range(S)]
        done, pos = [], [0] * S

        def push(entries, seed):
            streams = [e[0] for e in entries]
            chunks = [np.asarray(e[1], np.int16) for e in entries]
            fin = [int(bool(e[2])) for e in entries]
            want = [lv.window_count(s, c.size, f) for s, c, f in zip(streams, chunks, fin)]
            n = sum(want)
            pcm, offs, lens = pack(chunks, seed=seed, max_gap=9)
            d = torch.from_numpy(pcm).cuda()
            sc, rw = sentinel(n + PAD, 48), sentinel(n + PAD, 48)
            nw = lv.push_device(d.data_ptr(), streams, offs, lens, sc.data_ptr(), rw.data_ptr(), finish=fin)
            assert [int(x) for x in nw] == want
            sc, rw = host(sc), host(rw)
            assert untouched(sc[n:]) and untouched(rw[n:])
            at = 0
            for s, c, w, f in zip(streams, chunks, want, fin):
                life[s]["audio"] = np.concatenate([life[s]["audio"], c])
                life[s]["sc"] += list(sc[at:at + w])
                life[s]["rw"] += list(rw[at:at + w])
                at += w
                if f:
                    end(s, True)
            return want

        def end(s, finished):
            done.append(dict(life[s], finished=finished, stream=s))
            life[s] = dict(name=life[s]["name"], audio=np.zeros(0, np.int16), sc=[], rw=[], finished=False)

        def take(s, n, rec=None):
            rec = recs[s] if rec is None else rec
            c = rec[pos[s]:pos[s] + n]
            pos[s] += c.size
            return c
        assert push([(s, take(s, 3 * sl), False) for s in range(S)], 1) == [0] * S
        assert push([(s, take(s, sl + g), False) for s in range(S)], 2) == [1] * S
        push([(s, take(s, 2 * sl + 5), False) for s in range(S)], 3)
        push([(6, take(6, recs[6].size), True), (0, take(0, 100), False), (3, take(3, 0), False)], 4)          # stream 6 finishes
        end(7, False)
        lv.reset([7])
        lv.assign([7], [env.names.index("l1")])
        life[7]["name"], pos[7] = "l1", 0
        w = push([(7, take(7, 5 * sl + g, again), False), (1, take(1, sl), False), (5, take(5, sl), False)], 5)
        assert w[0] == 2
        push([(s, take(s, sl), False) for s in range(S) if s != 6], 6)
        push([(s, take(s, recs[s].size if s != 7 else again.size, None if s != 7 else again), True) for s in range(S) if s != 6], 7)
        assert len(done) == S + 1 and all(not v["sc"] for v in life)
        rows = sum(check_life(env, v["name"], v["audio"], v["sc"], v["rw"], v["finished"], sl, ("live", v["stream"], v["name"])) for v in done)
        seven = [v for v in done if v["stream"] == 7]
        assert [v["name"] for v in seven] == ["max", "l1"] and len(seven[0]["sc"]) >= 3 and len(seven[1]["sc"]) >= 3
        assert rows >= 30
    finally:
        lv.close()


# ---- banks ----------------------------------------------------------------------------------------------------------------------------------
def bank_routes(B):
    """one-hot routes (two rows per member), rows every member takes, rows nobody takes, and mixed masks"""
    r = np.zeros(B, np.uint32)
    r[:32] = np.uint32(1) << (np.arange(32, dtype=np.uint32) % 16)
    r[32:38] = 0xffff
    r[38:42] = 0
    r[42:] = np.random.default_rng(5).integers(1, 1 << 16, B - 42).astype(np.uint32)
    return r[np.random.default_rng(6).permutation(B)]


def check_bank(env, names, routes, out, rows_of, what):
    """member by member: the rows its bit routes to it against the restatement, every other word the sentinel"""
    B = routes.size
    for k, n in enumerate(names):
        at = np.nonzero((routes >> np.uint32(k)) & 1)[0]
        assert at.size >= 8
        got = host(out[k])
        assert_bits(got, expected(B + PAD, got.shape[1], list(zip(at, rows_of(n, at)))), what + (n,))


@pytest.mark.parametrize("width", ["49x13", "49x40"])
def test_routed_banks_of_corners_and_edge_models(width, pkg, envs, clips, cepstra):
    """a bank of the six corners and ten edge models: kws_bank_nn_mfma_routed_kernel with sixteen different plans in one launch, from audio
    and from the spiked cepstra; every routed (row, member) pair against the restatement, the rest the sentinel"""
    import torch
    env = envs(width)
    names = E.bank_names(width)
    bank = env.banks[width] = pkg.Bank([env.gm[n] for n in names])
    B = 48
    routes = bank_routes(B)
    assert (routes == 0).sum() == 4 and (routes == 0xffff).sum() == 6
    d = torch.from_numpy(clips[:B].copy()).cuda()
    out = [sentinel(B + PAD, env.gm[n].n_labels) for n in names]
    f = sentinel(B + PAD, env.F)
    bank.run_classifier_routed_device(d.data_ptr(), B, routes, [t.data_ptr() for t in out], f.data_ptr())
    s0, f0, _ = env.om[names[0]].run_batch(clips[:B], want_features=True)
    f = host(f)
    assert same(f[:B], f0) and untouched(f[B:])
    check_bank(env, names, routes, out, lambda n, at: env.om[n].run_batch(clips[at]), (width, "audio"))
    # every member takes every row (routes NULL)
    out = [sentinel(B + PAD, env.gm[n].n_labels) for n in names]
    bank.run_classifier_routed_device(d.data_ptr(), B, None, [t.data_ptr() for t in out], None)
    check_bank(env, names, np.full(B, 0xffff, np.uint32), out, lambda n, at: env.om[n].run_batch(clips[at]), (width, "audio, every member"))
    # the spiked cepstra
    m, want_f = cepstra(width)
    mfcc_d = torch.from_numpy(m[:B].copy()).cuda()
    out = [sentinel(B + PAD, env.gm[n].n_labels) for n in names]
    f = sentinel(B + PAD, env.F)
    bank.cmvn_inference_batch_device(mfcc_d.data_ptr(), B, [t.data_ptr() for t in out], f.data_ptr(), routes=routes)
    f = host(f)
    assert same(f[:B], want_f[:B]) and untouched(f[B:])
    for n in names:
        E.assert_rows_wrap(f[:B], *env.quant[n], (width, "bank", n))
    check_bank(env, names, routes, out, lambda n, at: np.stack([env.om[n].run_inference(f[r]) for r in at]), (width, "cepstra"))


# ---- the graphs outside the shape -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", ["49x13", "49x40"])
def test_graphs_outside_the_shape_are_refused_by_name_and_served_alone(width, pkg, envs, clips, cepstra):
    """a first block of 1 or 8 filters leaves 16-byte rows for the second block, which the matrix-core kernel does not read: kws_pool_create
    refuses such a member and names it; alone, each is served by kws_nn_kernel -- clips and spiked cepstra against the restatement"""
    import torch
    env = envs(width)
    B = 32
    d = torch.from_numpy(clips[:B].copy()).cuda()
    m, want_f = cepstra(width)
    mfcc_d = torch.from_numpy(m[:B].copy()).cuda()
    for n in E.OUTSIDE:
        gm, om = env.gm[n], env.om[n]
        with pytest.raises(pkg.KwsError) as e:
            pkg.Pool([env.gm["max"], env.gm["stock"], gm])
        assert e.value.code == UNSUPPORTED and "pool member 2" in str(e.value) and "kws_nn_kernel" in str(e.value), str(e.value)
        s, f = sentinel(B + PAD, gm.n_labels), sentinel(B + PAD, env.F)
        gm.run_classifier_batch_device(d.data_ptr(), B, s.data_ptr(), f.data_ptr())
        so, fo, _ = om.run_batch(clips[:B], want_features=True)
        s, f = host(s), host(f)
        assert same(s[:B], so) and same(f[:B], fo) and untouched(s[B:]) and untouched(f[B:]), (width, n)
        s, f = sentinel(B + PAD, gm.n_labels), sentinel(B + PAD, env.F)
        gm.cmvn_inference_batch_device(mfcc_d.data_ptr(), B, s.data_ptr(), f.data_ptr())
        s, f = host(s), host(f)
        assert same(f[:B], want_f[:B]) and untouched(s[B:]) and untouched(f[B:]), (width, n)
        assert same(s[:B], np.stack([om.run_inference(x) for x in f[:B]])), (width, n)
        E.assert_rows_wrap(f[:B], *env.quant[n], (width, n))
