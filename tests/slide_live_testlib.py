"""Helpers of the live one-shot window tests (kws_slide_live_*): streams fed from recordings push by push, every push checked on the spot
against the next rows of kws_slide_recordings_device on the stream's whole recording."""
import numpy as np

from kws_testlib import bits
from slide_testlib import MARGIN, SENTINEL, pack, slide, speech

AUTO, DIRECT, SHARED = 0, 1, 2


def windows_of(n, clip, hop):
    return 0 if n < clip else (n - clip) // hop + 1


def served(gm, hop, pre):
    """does the retained-row path serve this hop: a multiple of the frame stride, and windows that touch (include/kws/kws.h)"""
    st = gm.frame_stride_samples
    return hop % st == 0 and hop // st <= gm.n_frames - pre


def auto_path(gm, hop, pre):
    """AUTO's rule: SHARED where it is served and computes fewer rows per window than DIRECT"""
    return SHARED if served(gm, hop, pre) and hop // gm.frame_stride_samples + pre < gm.n_frames else DIRECT


def paths_for(gm, hop, pre):
    """the flags a session can be created with at this hop"""
    return [AUTO, DIRECT] + ([SHARED] if served(gm, hop, pre) else [])


def edge_lengths(clip, hop, long=40000):
    """eight recordings: around every edge of the window count, and about 2.5 s"""
    return [0, clip - 1, clip, clip + 1, clip + hop - 1, clip + hop, long, long - 3333]


class Reference:
    """the slide's rows for a set of recordings, computed once: per recording r, scores[r] [W_r][labels] and features[r] [W_r][F]"""

    def __init__(self, gm, recs, hop, flags=AUTO, seed=3):
        import torch
        self.recs = recs
        self.hop = hop
        self.pcm, self.offs, self.lens = pack(recs, seed=seed)
        self.d_pcm = torch.from_numpy(self.pcm).cuda()
        s, f, n = slide(gm, self.d_pcm, self.offs, self.lens, hop, flags)
        W = [windows_of(r.size, gm.clip_samples, hop) for r in recs]
        assert n == sum(W)
        cut = np.cumsum([0] + W)
        self.scores = [s[cut[i]:cut[i + 1]] for i in range(len(recs))]
        self.features = [f[cut[i]:cut[i + 1]] for i in range(len(recs))]
        self.W = W


class Feeder:
    """stream s of a session fed from ref.recs[rec_of[s]]; push() sends the next `length` samples of each named stream and checks the push:
    its counts against window_count and the window rule, its rows bitwise against the reference's next rows, the rows behind untouched"""

    def __init__(self, gm, sess, ref, rec_of=None, want_features=True, score_tol=None):
        """score_tol: scores within that of the reference's instead of bitwise (float32 graphs against the oracle)"""
        self.gm, self.sess, self.ref = gm, sess, ref
        self.score_tol = score_tol
        self.rec_of = list(range(len(ref.recs))) if rec_of is None else list(rec_of)
        self.pos = [0] * len(self.rec_of)
        self.got = [0] * len(self.rec_of)
        self.want_features = want_features
        self.pushes = 0

    def left(self, s):
        return self.ref.recs[self.rec_of[s]].size - self.pos[s]

    def restart(self, s, rec):
        """after a reset of stream s: it is fed from recording `rec` from its start"""
        self.rec_of[s] = rec
        self.pos[s] = self.got[s] = 0

    def push(self, entries):
        """entries: [(stream, length)]; returns the windows per entry"""
        import torch
        gm, ref = self.gm, self.ref
        clip, hop = gm.clip_samples, ref.hop
        streams = [s for s, _ in entries]
        lengths = [n for _, n in entries]
        assert all(0 <= n <= self.left(s) for s, n in entries)
        offs = [int(ref.offs[self.rec_of[s]]) + self.pos[s] for s in streams]
        want = [self.sess.window_count(s, n) for s, n in entries]
        assert want == [windows_of(self.pos[s] + n, clip, hop) - windows_of(self.pos[s], clip, hop) for s, n in entries]
        assert [windows_of(self.pos[s], clip, hop) for s in streams] == [self.got[s] for s in streams]
        total = sum(want)
        sc = torch.full((total + MARGIN, gm.n_labels), SENTINEL, dtype=torch.float32, device="cuda")
        ft = torch.full((total + MARGIN, gm.n_features), SENTINEL, dtype=torch.float32, device="cuda") if self.want_features else None
        nw = self.sess.push_device(ref.d_pcm.data_ptr(), streams, offs, lengths, sc.data_ptr(), ft.data_ptr() if self.want_features else None)
        torch.cuda.synchronize()
        self.pushes += 1
        assert [int(x) for x in nw] == want, (entries, nw, want)
        sc = sc.cpu().numpy()
        assert (sc[total:] == SENTINEL).all(), "scores written past the push's last window"
        if self.want_features:
            ft = ft.cpu().numpy()
            assert (ft[total:] == SENTINEL).all(), "features written past the push's last window"
        row = 0
        for (s, n), k in zip(entries, want):
            r, g = self.rec_of[s], self.got[s]
            if self.score_tol is None:
                assert (bits(sc[row:row + k]) == bits(ref.scores[r][g:g + k])).all(), ("scores", s, self.pos[s], n, g, k)
            elif k:
                assert np.abs(sc[row:row + k] - ref.scores[r][g:g + k]).max() <= self.score_tol, ("scores", s, self.pos[s], n, g, k)
            if self.want_features:
                assert (bits(ft[row:row + k]) == bits(ref.features[r][g:g + k])).all(), ("features", s, self.pos[s], n, g, k)
            row += k
            self.pos[s] += n
            self.got[s] += k
        return want

    def finished(self):
        """every stream has been fed its whole recording and has returned every window of it"""
        return all(self.left(s) == 0 and self.got[s] == self.ref.W[self.rec_of[s]] for s in range(len(self.rec_of)))

    def feed_randomly(self, rng, max_packet, subset=0.6, after_push=None):
        """random packets (1 sample .. max_packet, small ones as likely as large ones) to random subsets, until every recording is through;
        after_push(windows of the push) is called behind every push"""
        S = len(self.rec_of)
        while any(self.left(s) for s in range(S)):
            entries = []
            for s in rng.permutation(S):
                if rng.random() > subset:
                    continue
                kind = rng.integers(0, 4)
                n = int(rng.integers(1, 5)) if kind == 0 else int(rng.integers(1, 401)) if kind == 1 else int(rng.integers(1, max_packet + 1))
                entries.append((int(s), min(n, self.left(s))))
            got = self.push(entries)
            if after_push:
                after_push(sum(got))
        assert self.finished()


__all__ = ["AUTO", "DIRECT", "SHARED", "windows_of", "served", "auto_path", "paths_for", "edge_lengths", "Reference", "Feeder", "speech", "pack",
           "SENTINEL", "MARGIN"]
