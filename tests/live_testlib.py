"""Helpers of the live-stream tests (kws_live_*): reference windows from the recording scan, and a push driver that checks every push against
them as it goes -- the counts kws_live_window_count announced, the rows against the scan's next windows of each stream's recording, and that
nothing past the push's windows was written."""
import numpy as np

from kws_testlib import bits
from scan_testlib import SLICE, pack

SENTINEL = -7.0


def scan_windows(gm, recs, slice_samples=SLICE):
    """(scores, raw) [W][labels] per recording from one kws_scan_recordings_device call: the windows a live stream must return"""
    import torch
    pcm, offs, lens = pack(recs, seed=21)
    W = [gm.scan_window_count(int(n), slice_samples) for n in lens]
    n = sum(W)
    d = torch.from_numpy(pcm).cuda()
    s = torch.full((max(n, 1), gm.n_labels), SENTINEL, dtype=torch.float32, device="cuda")
    r = torch.full((max(n, 1), gm.n_labels), SENTINEL, dtype=torch.float32, device="cuda")
    gm.scan_recordings_device(d.data_ptr(), offs, lens, s.data_ptr(), r.data_ptr(), slice_samples=slice_samples)
    torch.cuda.synchronize()
    s, r = s.cpu().numpy()[:n], r.cpu().numpy()[:n]
    starts = np.concatenate([[0], np.cumsum(W)]).astype(np.int64)
    return [(s[starts[i]:starts[i + 1]], r[starts[i]:starts[i + 1]]) for i in range(len(recs))]


class LiveCheck:
    """A LiveStreams session whose every push is checked on the spot.  start(s, ref) gives stream s the reference windows of the recording
    it is about to receive (ref = (scores, raw) from scan_windows); push() hands host audio to the session (uploaded between noise, at odd
    offsets) and asserts, per entry: n_windows equals kws_live_window_count called before the push, the rows are bitwise the next windows
    of the stream's reference, a finish leaves none of the reference's windows missing; and that the output rows past the push's windows
    keep their sentinel.  got[s] collects the stream's (scores, raw) rows of its current recording."""

    def __init__(self, gm, n_streams, slice_samples=None, fast_counts=False):
        self.gm = gm
        self.lv = gm.live_streams(n_streams, slice_samples)
        self.ref = {}
        self.got = {}
        self.pushes = 0
        self.fast_counts = fast_counts
        self.fallbacks = self.exacts = 0

    def start(self, s, ref):
        self.ref[s] = ref
        self.got[s] = ([], [])

    def received(self, s):
        return sum(x.shape[0] for x in self.got[s][0])

    def push(self, entries, seed=None):
        """entries: [(stream, int16 samples, finish)].  Returns n_windows per entry."""
        import torch
        streams = [e[0] for e in entries]
        chunks = [np.asarray(e[1], np.int16) for e in entries]
        fin = [int(bool(e[2])) for e in entries]
        want = [self.lv.window_count(s, c.size, f) for s, c, f in zip(streams, chunks, fin)]
        n = sum(want)
        pcm, offs, lens = pack(chunks, seed=self.pushes if seed is None else seed, max_gap=9)
        d = torch.from_numpy(pcm).cuda()
        rows = n + 3
        sc = torch.full((rows, self.gm.n_labels), SENTINEL, dtype=torch.float32, device="cuda")
        rw = torch.full((rows, self.gm.n_labels), SENTINEL, dtype=torch.float32, device="cuda")
        nw = self.lv.push_device(d.data_ptr(), streams, offs, lens, sc.data_ptr(), rw.data_ptr(), finish=fin)
        self.pushes += 1
        assert [int(x) for x in nw] == want, (self.pushes, list(nw), want)
        torch.cuda.synchronize()
        sc, rw = sc.cpu().numpy(), rw.cpu().numpy()
        assert (sc[n:] == SENTINEL).all() and (rw[n:] == SENTINEL).all(), self.pushes
        if self.fast_counts:
            self.fallbacks += self.gm.fast_fallback_count()
            self.exacts += self.gm.fast_exact_count()
        pos = 0
        for s, w, f in zip(streams, want, fin):
            ref_s, ref_r = self.ref[s]
            k = self.received(s)
            assert k + w <= ref_s.shape[0], (self.pushes, s, k, w, ref_s.shape[0])
            assert (bits(sc[pos:pos + w]) == bits(ref_s[k:k + w])).all(), (self.pushes, s, k)
            assert (bits(rw[pos:pos + w]) == bits(ref_r[k:k + w])).all(), (self.pushes, s, k)
            self.got[s][0].append(sc[pos:pos + w])
            self.got[s][1].append(rw[pos:pos + w])
            pos += w
            if f:
                assert k + w == ref_s.shape[0], (self.pushes, s, k + w, ref_s.shape[0])
        return nw

    def result(self, s):
        """the stream's (scores, raw) of its current recording, concatenated"""
        L = self.gm.n_labels
        return (np.concatenate(self.got[s][0]).reshape(-1, L) if self.got[s][0] else np.zeros((0, L), np.float32),
                np.concatenate(self.got[s][1]).reshape(-1, L) if self.got[s][1] else np.zeros((0, L), np.float32))

    def close(self):
        self.lv.close()


def random_packets(rng, n, max_len=48000):
    """packet lengths covering n samples: half log-uniform over 1 .. max_len, half uniform (1 sample to 3 s at 16 kHz)"""
    out, left = [], n
    while left > 0:
        if rng.random() < 0.5:
            k = int(np.exp(rng.uniform(0.0, np.log(max_len))))
        else:
            k = int(rng.integers(1, max_len + 1))
        k = max(1, min(k, left))
        out.append(k)
        left -= k
    return out


def run_random_chunking(chk, recs, rng, subset_p=0.5):
    """every recording i to stream i in seeded random packets, each push to a random subset of the streams; a stream's last packet
    finishes it, or an extra zero-length push does"""
    plans = {i: random_packets(rng, r.size) for i, r in enumerate(recs)}
    pos = {i: 0 for i in plans}
    state = {i: "open" for i in plans}                 # open -> (all samples pushed, finish pending) -> done
    while any(v != "done" for v in state.values()):
        entries = []
        for i in plans:
            if state[i] == "done" or rng.random() >= subset_p:
                continue
            if state[i] == "pending":
                entries.append((i, recs[i][:0], True))
                state[i] = "done"
                continue
            if not plans[i]:                           # an empty recording: only a finish
                entries.append((i, recs[i][:0], True))
                state[i] = "done"
                continue
            k = plans[i].pop(0)
            chunk = recs[i][pos[i]:pos[i] + k]
            pos[i] += k
            last = not plans[i]
            fin = last and rng.random() < 0.5
            entries.append((i, chunk, fin))
            if last:
                state[i] = "done" if fin else "pending"
        if entries:
            order = rng.permutation(len(entries))
            chk.push([entries[j] for j in order])
