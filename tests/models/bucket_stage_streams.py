"""The sorted streams tests/test_gpu_bucket_stage.py runs stage 4 on and tests/test_bucket_stage_model_cpu.py checks the
queue bounds on.  A stream is built for the parameters of the merge form it runs in - `piece` partials per piece of a big
run, at most `nb` buckets per window - and carries its own launch parameters:
  W, n, K, chunks_per_window, windows (W lists of n (digit, sign, base index)), zstart, scalars (the bases as integers,
  tests/models/bucket_stage_model.py), overrides [walk, run_lanes, big_chunks, block cap] (0 = the plan's value)
Every run is placed by the number of chunks it continues into (L = last - lane): it starts at the LAST entry of a chunk and
ends `e` entries into chunk lane + L; filler buckets of one to three entries bring the next run to the last entry of a
chunk again - of the same chunk where they fit, so that chunks hold a head and a tail partial at once."""
import random

POOL = [0, 1, 2, 3, 5, 7, 11, 13, 200]     # scalars[i]: base i = POOL[i] * generator; base 0 is the identity
WALK, BIG = 4, 32                          # the routing the placed streams are laid out for (walk: merge_plan's own)


class _Window:
    def __init__(self, K, nb, rnd, identities=False):
        self.K, self.nb, self.rnd, self.identities = K, nb, rnd, identities
        self.entries, self.digit, self.spare = [], 0, nb

    def _next_digit(self):
        # leave a bucket empty now and then, while there are digits to spare
        self.digit += 2 if (self.spare > 200 and self.digit % 3 == 1) else 1
        assert self.digit <= self.nb, "out of buckets"
        return self.digit

    def _base(self):
        lo = 0 if (self.identities and self.rnd.randrange(6) == 0) else 1
        return self.rnd.randrange(2), self.rnd.randrange(lo, len(POOL))

    def filler(self, count):
        """buckets of one to three entries - where buckets are scarce, one bucket"""
        while count:
            take = count if self.nb <= 128 else min(count, self.rnd.randrange(1, 4))
            d = self._next_digit()
            self.entries += [(d,) + self._base() for _ in range(take)]
            count -= take

    def to_chunk_end(self):
        """fill up to the last entry of the current chunk"""
        self.filler((self.K - 1 - len(self.entries)) % self.K)

    def run(self, L, e, pattern="mixed"):
        """a run that starts here - the last entry of a chunk - continues into L chunks and has e entries in the last"""
        K = self.K
        assert len(self.entries) % K == K - 1 and L >= 1 and 1 <= e <= K
        count = 1 + (L - 1) * K + e
        d = self._next_digit()
        b = self.rnd.randrange(1, len(POOL))
        if pattern == "mixed":
            new = [(d,) + self._base() for _ in range(count)]
        elif pattern == "single":      # equal partials: every level of a merge tree doubles
            new = [(d, 0, b)] * count
        elif pattern == "alternate":   # P, then -P, P, ...: the first partial is P, the full chunks cancel
            new = [(d, i & 1, b) for i in range(count)]
        elif pattern == "alternate0":  # an identity base first, then P, -P, ...: every partial of full chunks is the identity
            new = [(d, 0, 0)] + [(d, i & 1, b) for i in range(count - 1)]
        else:                          # "halves": the partials of the first half are multiples of P, of the second of -P
            new = [(d, 1 if i >= count // 2 else 0, b) for i in range(count)]
        self.entries += new


def _placed_window(K, nb, rnd, runs, identities=False, lead=0, total=None):
    """runs: [(L, pattern)]; the last run ends at the last entry of the window, which is no multiple of K.  total: one more
    run brings the window to that many entries"""
    w = _Window(K, nb, rnd, identities)
    for _ in range(lead):
        w.filler(K)
    w.filler(K - 1)
    for i, (L, pattern) in enumerate(runs):
        e = 1 + (i * 3 + 2) % (K - 1)      # 1 .. K - 1, all of them over a window
        w.run(L, e, pattern)
        if i + 1 < len(runs) or total:
            w.to_chunk_end()
    if total:
        rest = total - len(w.entries)
        L = (rest - 2) // K + 1
        w.run(L, rest - 1 - (L - 1) * K, "mixed")
        assert len(w.entries) == total
    return w.entries


def _finish(name, K, lives, zs, overrides, rnd, chunks_per_window=None):
    """pad every window to the common n with entries below z whose digit is the first live digit"""
    n = max(len(e) + z for e, z in zip(lives, zs))
    windows, zstart = [], []
    for live, z in zip(lives, zs):
        z = n - len(live)
        first = live[0][0] if live else 1
        windows.append([(first, rnd.randrange(2), rnd.randrange(len(POOL))) for _ in range(z)] + live)
        zstart.append(z)
    cpw = chunks_per_window or (n + K - 1) // K
    return dict(name=name, W=len(windows), n=n, K=K, chunks_per_window=cpw, windows=windows, zstart=zstart, scalars=POOL,
                overrides=overrides)


def boundaries(piece, nb, branches=False):
    """K = 8, two windows with different streams and different z.  L: 1, 2, walk, walk + 1, walk + 2, big, big + 1 in both;
    piece - 1 and 2 piece (piece and 2 piece + 1 partials) in the first, piece and 2 piece - 1 in the second"""
    rnd = random.Random("bucket stage %s %d" % ("branches" if branches else "boundaries", piece))
    K = 8
    small = [1, 2, WALK, WALK + 1, WALK + 2, BIG, BIG + 1]
    if branches:
        pat0 = {BIG + 1: "alternate0", WALK + 2: "alternate", BIG: "single", piece - 1: "halves", WALK + 1: "halves", 2: "single"}
        pat1 = {BIG + 1: "single", WALK + 1: "alternate", BIG: "halves", piece: "alternate0", 1: "single"}
    else:
        pat0 = pat1 = {}
    runs0 = [(L, pat0.get(L, "mixed")) for L in small[:4] + [piece - 1] + small[4:] + [2 * piece]]
    runs1 = [(L, pat1.get(L, "mixed")) for L in [BIG + 1, piece] + small[:6][::-1] + [2 * piece - 1]]
    lives = [_placed_window(K, nb, rnd, runs0, branches), _placed_window(K, nb, rnd, runs1, branches, lead=1)]
    assert len(lives[0]) != len(lives[1]) and all(len(e) % K for e in lives)
    n = max(len(e) for e in lives) + 13
    return _finish("branches" if branches else "boundaries", K, lives, [n - len(e) for e in lives], [0, 0, BIG, 0], rnd)


def effective_k32(piece, nb):
    """plan K = 32 over three windows: an effective chunk of 13; so few live entries that the floor of 8 leaves most lanes
    without a chunk; z = n"""
    rnd = random.Random("bucket stage effective %d" % piece)
    cpw, Ke = 300, 13
    n = 32 * cpw - 5
    runs = [(L, "mixed") for L in (WALK + 1, 1, BIG + 1, WALK, BIG, 2, WALK + 2)]
    live0 = _placed_window(Ke, nb, rnd, runs, total=Ke * cpw - 7)       # ceil(live / cpw) = 13
    live1 = _placed_window(8, nb, rnd, [(L, "mixed") for L in (WALK, WALK + 1, 3, BIG + 1)])
    assert (len(live1) + cpw - 1) // cpw < 8 and (len(live1) + 7) // 8 < cpw
    s = _finish("effective-K32", 32, [live0, live1, []], [n - len(live0), n - len(live1), n], [0, 0, BIG, 0], rnd, cpw)
    assert s["n"] == n
    return s


def effective_k4(piece, nb):
    """plan K = 4, below the floor of 8: the effective chunk is 4"""
    rnd = random.Random("bucket stage k4 %d" % piece)
    lives = [_placed_window(4, nb, rnd, [(L, "mixed") for L in order]) for order in
             ((1, WALK, BIG + 1, WALK + 1, 2, BIG), (WALK + 2, BIG, 1, WALK + 1, WALK, BIG + 1))]
    n = max(len(e) for e in lives) + 6
    return _finish("effective-K4", 4, lives, [n - len(e) for e in lives], [0, 0, BIG, 0], rnd)


LOOPS_WALK, LOOPS_BIG, LOOPS_MEDIUM = 2, 8, 37


def loops(piece, nb):
    """one window, walk 2 and big_chunks 8, one workgroup for the medium runs (four wavefronts) and two for the pieces:
    37 medium runs - more than a round of the four wavefronts at any G, and no multiple of a wavefront's share - and five
    big runs of 2 + 1 + 2 + 1 + 1 pieces"""
    rnd = random.Random("bucket stage loops %d" % piece)
    runs = [(LOOPS_WALK + 1 + i % (LOOPS_BIG - LOOPS_WALK), "mixed") for i in range(LOOPS_MEDIUM)]
    big = [piece, LOOPS_BIG + 1, piece + 3, LOOPS_BIG + 2, piece - 1]
    for i, L in enumerate(big):
        runs.insert(3 + 7 * i, (L, "mixed"))
    live = _placed_window(8, nb, rnd, runs)
    return _finish("loops", 8, [live], [5], [LOOPS_WALK, 0, LOOPS_BIG, 1], rnd)


def skewed(seed, piece, nb):
    """skewed digits, random z, production routing"""
    rnd = random.Random("bucket stage random %d" % seed)
    K = (4, 8, 16)[seed % 3]
    W = 2
    lives = []
    for _ in range(W):
        nd = rnd.randrange(12, min(nb, 40))
        digits = sorted(rnd.sample(range(1, nb + 1), nd))
        live = []
        for d in digits:
            r = rnd.randrange(10)
            count = rnd.randrange(1, 4) if r < 5 else rnd.randrange(4, 6 * K) if r < 8 else rnd.randrange(6 * K, 80 * K)
            live += [(d, rnd.randrange(2), rnd.randrange(len(POOL))) for _ in range(count)]
        lives.append(live)
    n = max(len(e) for e in lives) + rnd.randrange(1, 50)
    return _finish("random%d" % seed, K, lives, [n - len(e) for e in lives], [0, 0, 0, 0], rnd)


def all_streams(piece, nb):
    return [boundaries(piece, nb), boundaries(piece, nb, True), effective_k32(piece, nb), effective_k4(piece, nb), loops(piece, nb)] + \
           [skewed(s, piece, nb) for s in range(3)]


STREAM_NAMES = ["boundaries", "branches", "effective-K32", "effective-K4", "loops", "random0", "random1", "random2"]


def window_bits(W, small):
    """c: the largest with W 2^(c-1) <= 128 buckets for the forms that need a small set, else 9"""
    if not small:
        return 9
    c = 2
    while W << c <= 128:
        c += 1
    return c


# ------------------------------------------------------------------------------------------ adversarial streams (bounds)
def packed(K, L, nchunks):
    """live entries over nchunks chunks of K: runs that continue into L chunks packed back to back - each starts at the last
    entry of a chunk and ends at the first entry of chunk lane + L, one filler bucket of K - 2 entries in between"""
    entries, d = [(1, 0, 1)] * (K - 1), 1
    per_run = 1 + (L - 1) * K + 1
    while len(entries) + per_run <= nchunks * K:
        d += 1
        entries += [(d, 0, 1)] * per_run
        if len(entries) + K - 2 > nchunks * K:
            break
        d += 1
        entries += [(d, 0, 1)] * (K - 2)
    return entries


def one_run(K, nchunks):
    return [(1, 0, 1)] * (nchunks * K - 3)


# ------------------------------------------------------------------------------------- the streams of a merge form, once
_BUILDERS = [("boundaries", 2, boundaries), ("branches", 2, lambda piece, nb: boundaries(piece, nb, True)),
             ("effective-K32", 3, effective_k32), ("effective-K4", 2, effective_k4), ("loops", 1, loops)] + \
            [("random%d" % s, 2, (lambda s: lambda piece, nb: skewed(s, piece, nb))(s)) for s in range(3)]
assert [b[0] for b in _BUILDERS] == STREAM_NAMES
_built = {}


def stream(name, piece, small):
    """the stream `name` for a merge form with `piece` partials per piece; small: the form needs at most 128 buckets in all.
    Adds c, the window bits it is laid out for"""
    key = (name, piece, small)
    if key not in _built:
        _, W, build = _BUILDERS[STREAM_NAMES.index(name)]
        c = window_bits(W, small)
        s = build(piece, 1 << (c - 1))
        assert s["W"] == W and s["n"] <= s["chunks_per_window"] * s["K"]
        s["c"] = c
        _built[key] = s
    return _built[key]
