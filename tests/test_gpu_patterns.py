"""The entropy coders on CHOSEN symbol patterns: bursts, silence, stream tails.

Every other coder test feeds the kernels KV drawn from randn / rand / outlier: each lane of a stream then emits a word
every four or five tokens, out of phase with its neighbours -- a steady trickle of 15 to 20 words per token.  Byte
equality with the oracle on such data shows that the GPU does the oracle's arithmetic; it says little about what only
the kernels have: the encoder's linear 256-word staging buffer (flush test every second token, pieces on a 256-byte
grid, a masked first piece, the stream's end in two dword-per-lane pieces: k_encode_counts.h, k_encode.h, k_fused.h),
the decoder's two-block word ring (looked after behind every second token: k_decode.h) and the placement of streams
before they are coded.  Here the quantiser is held fixed -- KV of exact small integers whose row maximum is the
quantiser's MAX, so factor = 1 and the symbols are the ones written down -- and the SYMBOLS are chosen:

  bursts    the 64 lanes of a stream in lockstep: 64 words at one token, again at the next or the one after it
  silence   streams without a single word (top_blk = -1, nothing flushed, the first masked piece is also the last)
  tails     every word count mod 128, every pair of (where a stream starts, where it ends) on the 256-byte grid

The patterns are DEFINED by how many words a stream takes at each token (the oracle's trace, lmco_trace_group_words);
what a pattern is meant to reach is asserted from that trace and from the oracle's blobs on the CPU, before anything
runs on the GPU.  On the GPU every blob of both launch paths is byte-equal to the oracle's and every decode bit-equal:
there are no tolerances in this file.  The CPU parts are not marked `gpu` and run everywhere."""
import functools
import struct

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda:0"
D = 128                # head size of every job here; C = 128 (one head) or 384 (three)
BINS = (32, 16)        # K plane: 31 symbols (the decoder's narrow search, byte workspace); V plane: 15 symbols (wide
                       # search, nibble workspace) -- every chunk carries both
EXTRA_LANES = (5, 13, 22, 31, 40, 47, 58, 62)  # the lanes that leave the lockstep to move a run along the stream


def _oracle():
    """The CPU oracle (test infrastructure), built if stale -- what conftest's `oracle` fixture returns."""
    from oracle import lmc_oracle
    lmc_oracle.build()
    return lmc_oracle


# ---------------------------------------------------------------------------------------------------------------
# 1. KV from a symbol table
# ---------------------------------------------------------------------------------------------------------------
def kv_from_symbols(sym, bins, dtype, head_size=D):
    """KV [L, 2, T, H, D] in `dtype` whose quantisation IS the table sym [P, T, C] (plane p = kv * L + layer).

    With MAX = bins // 2 - 1 the values are the exact small integers x = sym - MAX.  Every token row of every plane must
    hold the top symbol 2 * MAX somewhere (the jobs below reserve the plane's last channel for it, outside the groups
    under test): the row maximum is then MAX, the quantiser's factor MAX / max is exactly 1.0, round(x * 1 + MAX) = sym,
    and the scale is the constant MAX.  Asserted against oracle.quantize before the KV is handed out.  bf16, fp16 and
    float8_e4m3fn hold every integer up to 15; float8_e5m2 does not (two mantissa bits) and is refused."""
    oracle = _oracle()
    sym = np.ascontiguousarray(sym, np.int8)
    bins = np.asarray(bins, np.int32)
    P, T, C = sym.shape
    L = P // 2
    assert dtype in (torch.bfloat16, torch.float16, torch.float8_e4m3fn), f"{dtype} cannot hold the integers up to 15"
    assert bins.shape == (P,) and P == 2 * L and C % head_size == 0 and all(int(b) in (16, 32) for b in bins)
    mx = (bins // 2 - 1).astype(np.int64)
    assert sym.min() >= 0 and (sym <= 2 * mx[:, None, None]).all()
    assert (sym == 2 * mx[:, None, None]).any(axis=2).all(), "a token row without the reserved top symbol: its factor is not 1"
    x = sym.astype(np.float32) - mx[:, None, None].astype(np.float32)
    kv = torch.from_numpy(x).reshape(2, L, T, C).permute(1, 0, 2, 3).contiguous().to(dtype)
    img = kv.to(torch.bfloat16) if dtype == torch.float8_e4m3fn else kv  # (an fp8 chunk is coded as its bf16 images)
    assert torch.equal(img.float(), torch.from_numpy(x).reshape(2, L, T, C).permute(1, 0, 2, 3)), "not exact in this dtype"
    bits, code = oracle.torch_to_bits(img)
    got, scale = oracle.quantize(bits, code, bins)
    assert np.array_equal(got, sym), "the quantiser does not return the symbol table"
    want_scale = oracle.torch_to_bits(torch.from_numpy(mx.astype(np.float32)).to(img.dtype))[0]
    assert (scale == want_scale[:, None]).all(), "the scale is not the constant MAX"
    return kv.reshape(L, 2, T, C // head_size, head_size)


# ---------------------------------------------------------------------------------------------------------------
# 2. words per token, and what a blob's directory says
# ---------------------------------------------------------------------------------------------------------------
def stream_table(oracle, blob, base=0):
    """Per stream of a blob that lies at byte `base` of its arena: (begin, head bytes, words in front of the 64 states,
    end), begin and end as ARENA offsets (end exact: behind the last state word).  From the header, the stream directory
    and the widths at the front of each head (lmc_format.h)."""
    h = oracle.parse_header(blob)
    out = []
    for pg, (beg, end) in enumerate(oracle.stream_dir(blob)):
        R = blob[h["off_bins"] + pg // h["ngroups"]] - 1
        R8 = (R + 7) & ~7
        at = h["off_streams"] + int(beg)
        hb = (R8 + 8 * sum(blob[at:at + R8]) + 15) & ~15
        nw, odd = divmod(int(end - beg) - hb - 4 * 64, 2)
        assert nw >= 0 and not odd
        out.append((base + at, hb, nw, base + h["off_streams"] + int(end)))
    return out


def longest_alternation(tr):
    """Tokens of the longest run in which every second token takes 64 words (m such tokens two apart: 2 m tokens)."""
    best = 0
    for par in (0, 1):
        m = 0
        for v in tr[par::2]:
            m = m + 1 if v == 64 else 0
            best = max(best, m)
    return 2 * best


def has_pair(tr):
    """Two CONSECUTIVE tokens that take 64 words each."""
    return bool(((tr[:-1] == 64) & (tr[1:] == 64)).any())


def window3(tr):
    """The most words any three consecutive tokens take."""
    return int((tr[:-2] + tr[1:-1] + tr[2:]).max()) if len(tr) >= 3 else int(tr.sum())


# ---------------------------------------------------------------------------------------------------------------
# 3. pattern families.  A group is an int8 table [T, 64] of one stream's lanes; a plane is its groups side by side.
# ---------------------------------------------------------------------------------------------------------------
def busy_group(rng, T, R):
    """What the other tests feed the coders: every lane draws its symbols independently (a trickle of words)."""
    return rng.integers(0, R, (T, 64)).astype(np.int8)


def silent_group(T, R, g):
    """Every lane constant (lane by lane another symbol, symbol 0 and the top one among them): head + states, no word."""
    return np.repeat(((np.arange(64) * 7 + 3 * g) % R).astype(np.int8)[None, :], T, 0)


def plane_of(groups, R):
    """Groups side by side; the plane's LAST channel is the reserved one (the top symbol on every token)."""
    pl = np.concatenate(groups, axis=1)
    pl[:, -1] = R - 1
    return pl


def lockstep_column(T, R, a, uniform=False):
    """One lane of a lockstep stream.  uniform: the R symbols in turn.  Otherwise the R - 1 symbols other than the
    constant c = R // 2 once each at tokens [a, a + R - 1) -- a symbol that occurs once costs 8 bits at T = 256, 11 at
    T = 2048 -- and c everywhere else.  The run's top token carries c + 1 and its bottom token c - 1: an extra lane that
    repeats THOSE symbols above the run changes no other symbol's frequency (only the cumulative count at c moves)."""
    if uniform or T < R:
        return (np.arange(T) % R).astype(np.int8)
    c = R // 2
    col = np.full(T, c, np.int8)
    col[a:a + R - 1] = [c - 1] + list(range(c + 2, R)) + list(range(0, c - 1)) + [c + 1]
    return col


def burst_group(T, R, a, k=0, q=(0, 0)):
    """64 lanes in lockstep on lockstep_column; k of them (EXTRA_LANES) also carry, at the tokens right above the run, q[0]
    times the run's top symbol and q[1] times its bottom symbol: a few more words in front of the run (in stream order),
    nothing else changed."""
    col = lockstep_column(T, R, a)
    g = np.repeat(col[:, None], 64, 1)
    if k:
        pos = a + R + np.arange(q[0] + q[1])
        assert pos[-1] < T
        g[np.ix_(pos, EXTRA_LANES[:k])] = np.array([R // 2 + 1] * q[0] + [R // 2 - 1] * q[1], np.int8)[:, None]
    return g


@functools.lru_cache(maxsize=None)
def burst_family(T, bins, where):
    """The lockstep run at the chunk's `where` (start / middle / end), at eight offsets in the stream.

    The decoder's ring and the encoder's staging buffer see a run at the stream position of its first word: e = the words
    the tokens ABOVE the run take (the encoder walks the tokens downwards, the decoder pops from the stream's end).  In
    lockstep e is a multiple of 64, so k = 0 .. 7 lanes take w more words up there each.  A lane that has coded other
    symbols arrives at the run in another state, and whether it still renormalises at the tokens the others do is a matter
    of that state: the generator SEARCHES the start token a and the numbers q of repeated symbols for a lane whose trace
    over the run is the lockstep lanes' own (lanes are independent: what holds for one extra lane holds for k), and
    keeps the first hit whose offsets e + k w are distinct mod 128.  -> ([group of k = 0 .. 7], a, offsets).
    `end`: the run is the first thing the encoder codes, e = 0 whatever the lanes do: one group."""
    oracle = _oracle()
    R, n1 = bins - 1, bins - 2
    trace = lambda g: oracle.trace_group_words(np.ascontiguousarray(g), 0, bins)
    if where == "end":
        return [burst_group(T, R, T - n1)], T - n1, [0]
    a0 = 0 if where == "start" else (T - n1) // 2
    qmax = min(48, (T - a0 - R - 4) // 2)
    for a in range(a0, a0 + 4):
        base = trace(burst_group(T, R, a))
        e0 = int(base[a + n1:].sum())
        for q in sorted(((q0, q1) for q0 in range(qmax + 1) for q1 in range(qmax + 1) if q0 + q1), key=lambda q: (q[0] + q[1], q[1])):
            tr = trace(burst_group(T, R, a, 1, q))
            w = int(tr[a + n1:].sum()) - e0
            if np.array_equal(tr[a:a + n1], base[a:a + n1]) and w >= 1 and len({(e0 + k * w) % 128 for k in range(8)}) == 8:
                groups = [burst_group(T, R, a, k, q) for k in range(8)]
                offs = []
                for g in groups:  # (computed from each group's own trace, not from the arithmetic above)
                    t = trace(g)
                    assert np.array_equal(t[a:a + n1], base[a:a + n1]), "an extra lane left the lockstep inside the run"
                    offs.append(int(t[a + n1:].sum()) % 128)
                assert len(set(offs)) == 8, offs
                return groups, a, offs
    raise AssertionError(f"no lockstep run at {where} of T = {T}, {bins} bins keeps its 64-word tokens at 8 offsets: the generator is wrong")


class Job:
    """One encode launch: n chunks of T tokens, L = 1 (plane 0 = K with BINS[0], plane 1 = V with BINS[1]), C channels.
    chunks: [n][2] planes [T, C]; streams: {(chunk, plane, group): (family, tag)} of the streams under test."""

    def __init__(self, name, T, C, dtype, chunks, streams):
        self.name, self.T, self.C, self.dtype, self.streams = name, T, C, dtype, streams
        self.sym = np.ascontiguousarray(np.stack([np.stack(c) for c in chunks]), np.int8)  # [n, 2, T, C]
        self.n, self.H, self.G = len(chunks), C // D, C // 64

    def table(self):
        """The job's symbol table [2, n T, C]."""
        return np.ascontiguousarray(self.sym.transpose(1, 0, 2, 3).reshape(2, self.n * self.T, self.C))

    def kv(self, dtype=None):
        return kv_from_symbols(self.table(), BINS, dtype or self.dtype)

    def stride(self, oracle):
        return (oracle.blob_bound(1, self.T, self.H, D) + 15) & ~15

    @functools.lru_cache(maxsize=None)
    def refs(self, model=-1):
        """The oracle's blob of every chunk (computed once, shared by the tests)."""
        oracle = _oracle()
        bits, code = oracle.torch_to_bits(self.kv(torch.float16 if self.dtype == torch.float16 else torch.bfloat16)
                                          .reshape(1, 2, self.n * self.T, self.C))
        return [oracle.encode_blob(bits[:, :, i * self.T:(i + 1) * self.T], code, self.H, D, np.array(BINS, np.int32), model)
                for i in range(self.n)]

    @functools.lru_cache(maxsize=None)
    def want(self, out_code, model=-1):
        """oracle.decode_blob of every chunk, side by side: uint16 [1, 2, n T, C]."""
        oracle = _oracle()
        return np.concatenate([oracle.decode_blob(b, out_code) for b in self.refs(model)], axis=2)

    def words(self, oracle, chunk, p, g):
        return oracle.trace_group_words(self.sym[chunk, p], g, BINS[p])


SILENCE_SHAPES = ("all silent", "alternating", "alternating, the other way", "first and last stream silent")


def silence_chunks(rng, T, C, first_chunk):
    """The three job shapes of the silence family (the alternation both ways round), one chunk each."""
    G = C // 64
    chunks, streams = [], {}
    for i, shape in enumerate(SILENCE_SHAPES):
        planes = []
        for p, bins in enumerate(BINS):
            R = bins - 1
            silent = {"all silent": lambda g: True, "alternating": lambda g: (g + p) % 2 == 0,
                      "alternating, the other way": lambda g: (g + p) % 2 == 1,
                      "first and last stream silent": lambda g: (p, g) in ((0, 0), (1, G - 1))}[shape]
            groups = []
            for g in range(G):
                groups.append(silent_group(T, R, g) if silent(g) else busy_group(rng, T, R))
                if silent(g):
                    streams[(first_chunk + i, p, g)] = ("silence", shape)
            planes.append(plane_of(groups, R))
        chunks.append(planes)
    return chunks, streams


@functools.lru_cache(maxsize=None)
def pattern_job(T, C, dtype):
    """Bursts and silence as chunks of ONE job, so that a launch holds many streams and the look-back carries extreme
    stream lengths side by side.  Per plane the variants are the run at the start and in the middle at 8 offsets each, the
    run at the end, and the uniform lockstep: 18 streams under test, in the groups in front of the plane's last (which
    holds the reserved channel and otherwise a busy trickle)."""
    rng = np.random.default_rng(1000 * T + C)
    G = C // 64
    slots = G - 1
    per_plane = []
    for bins in BINS:
        R = bins - 1
        if T < R:  # T = 1: a chunk is one token, every stream is one symbol per lane and takes no word
            v = [(np.full((T, 64), s % R, np.int8), ("burst", f"T{T} all lanes symbol {s % R}", 0)) for s in (0, R // 2, R - 1)]
            v.append((busy_group(rng, T, R), ("burst", f"T{T} a symbol per lane", 0)))
        else:
            v = []
            for where in ("start", "middle", "end"):
                groups, a, offs = burst_family(T, bins, where)
                v += [(g, ("burst", f"run at {where} (token {a}), {k} extra lanes", off)) for k, (g, off) in enumerate(zip(groups, offs))]
            v.append((np.repeat(lockstep_column(T, R, 0, uniform=True)[:, None], 64, 1), ("burst", "uniform lockstep", 0)))
        per_plane.append(v)
    nvar = len(per_plane[0])
    nchunks = (nvar + slots - 1) // slots
    chunks, streams = [], {}
    for i in range(nchunks):
        planes = []
        for p, bins in enumerate(BINS):
            R = bins - 1
            groups = []
            for g in range(slots):
                grp, tag = per_plane[p][(i * slots + g) % nvar]  # (spare slots of the last chunk repeat the first variants)
                groups.append(grp)
                streams[(i, p, g)] = tag
            groups.append(busy_group(rng, T, R))
            planes.append(plane_of(groups, R))
        chunks.append(planes)
    sc, ss = silence_chunks(rng, T, C, nchunks)
    streams.update(ss)
    return Job(f"T{T}_C{C}", T, C, dtype, chunks + sc, streams)


# (T, C, dtype of the KV).  T = 256 / 100: counts model, plain and scaled; 300 / 2048 / 1: CDF16.  C = 128: narrow planes,
# several per fused work item, histogram read from the workspace; C = 384: one plane per item, histogram in LDS.
PATTERN_JOBS = [(256, 128, torch.bfloat16), (256, 384, torch.float16), (100, 128, torch.float16), (100, 384, torch.bfloat16),
                (300, 128, torch.bfloat16), (300, 384, torch.float16), (2048, 128, torch.bfloat16),
                (1, 128, torch.bfloat16), (1, 384, torch.float16)]
PATTERN_IDS = [f"T{t}_C{c}" for t, c, _ in PATTERN_JOBS]


TAIL_JOBS = [(256, 384, torch.bfloat16), (64, 384, torch.float16), (100, 384, torch.bfloat16), (300, 128, torch.bfloat16)]
TAIL_IDS = [f"tails_T{t}_C{c}" for t, c, _ in TAIL_JOBS]
TAIL_CHUNKS = 64


@functools.lru_cache(maxsize=None)
def tail_job(T, C, dtype):
    """64 chunks whose streams' word counts are steered by (busy lanes) x (costly tokens): b lanes, 0 .. 64 in turn,
    carry a symbol drawn per lane at m of the chunk's tokens and a constant elsewhere; the other lanes are constant."""
    rng = np.random.default_rng(77 * T + C)
    G = C // 64
    chunks, streams, turn = [], {}, 0
    for i in range(TAIL_CHUNKS):
        planes = []
        for p, bins in enumerate(BINS):
            R = bins - 1
            groups = []
            for g in range(G):
                b, m = turn % 65, int(rng.integers(1, min(T, 48) + 1))
                turn += 1
                grp = silent_group(T, R, g)
                lanes = rng.permutation(64)[:b]
                toks = np.sort(rng.permutation(T)[:m])
                grp[np.ix_(toks, lanes)] = rng.integers(0, R, (m, b))
                groups.append(grp)
                streams[(i, p, g)] = ("tails", f"{b} busy lanes x {m} tokens")
            planes.append(plane_of(groups, R))
        chunks.append(planes)
    return Job(f"tails_T{T}_C{C}", T, C, dtype, chunks, streams)


def tail_coverage(oracle, jobs):
    """From the oracle blobs' directories, every stream at its place in the job's arena (chunk i at i * stride, the arena
    itself 256-byte aligned -- the GPU test asserts that of its buffer): the word counts mod 128 that occur, and the pairs
    (stream start mod 256) / 16, (end of the stream's last state word mod 256) / 16."""
    mods, pairs, nstreams = set(), set(), 0
    for job in jobs:
        stride = job.stride(oracle)
        for i, blob in enumerate(job.refs()):
            for beg, hb, nw, end in stream_table(oracle, blob, i * stride):
                mods.add(nw % 128)
                pairs.add(((beg % 256) // 16, (end % 256) // 16))
                nstreams += 1
    return mods, pairs, nstreams


# ---------------------------------------------------------------------------------------------------------------
# CPU tests
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float8_e4m3fn], ids=["bf16", "fp16", "e4m3"])
def test_kv_from_symbols_is_the_quantisers_fixed_point(oracle, dtype):
    """The helper's own assertion (oracle.quantize returns the table, the scale is MAX) on tables that use every symbol of
    16- and 32-bin planes, two layers; and the blob of such KV decodes to the table again."""
    rng = np.random.default_rng(5)
    bins = [32, 16, 16, 32]
    T, C = 37, 256
    sym = np.stack([rng.integers(0, b - 1, (T, C)) for b in bins]).astype(np.int8)
    for p, b in enumerate(bins):
        sym[p, :, 0] = np.arange(T) % (b - 1)   # every symbol occurs
        sym[p, :, -1] = b - 2                   # the reserved channel
    kv = kv_from_symbols(sym, bins, dtype)
    assert kv.shape == (2, 2, T, 2, D) and kv.dtype == dtype
    img = kv.to(torch.bfloat16) if dtype == torch.float8_e4m3fn else kv
    bits, code = oracle.torch_to_bits(img.reshape(2, 2, T, C))
    blob = oracle.encode_blob(bits, code, 2, D, np.array(bins, np.int32))
    assert np.array_equal(oracle.decode_blob_symbols(blob), sym)
    with pytest.raises(AssertionError):
        kv_from_symbols(sym, bins, torch.float8_e5m2)
    bad = sym.copy()
    bad[1, 5, -1] = 3  # a row without the top symbol: refused, not silently rescaled
    bad[1, 5][bad[1, 5] == 14] = 0
    with pytest.raises(AssertionError):
        kv_from_symbols(bad, bins, dtype)


@pytest.mark.parametrize("T,model", [(256, -1), (100, -1), (300, -1), (1, -1), (256, 0), (100, 0)],
                         ids=["T256", "T100", "T300", "T1", "T256_cdf16", "T100_cdf16"])
def test_trace_sums_to_the_directory(oracle, T, model):
    """Words per token (lmco_trace_group_words) against the blob: per stream the trace's sum is the word count the
    directory and the head give -- on a random chunk (KV from randn through the quantiser) and on a patterned one."""
    C, H = 192, 3
    g = torch.Generator().manual_seed(T)
    kv = torch.randn(1, 2, T, C, generator=g).to(torch.bfloat16)
    bits, code = oracle.torch_to_bits(kv)
    cases = [("random", bits, code, oracle.quantize(bits, code, np.array(BINS, np.int32))[0], H, 64)]
    job = pattern_job(*next(j for j in PATTERN_JOBS if j[:2] == (T, 128)))
    jb, jc = oracle.torch_to_bits(job.kv().reshape(1, 2, job.n * T, 128)[:, :, :T].contiguous())
    cases.append(("patterned", jb, jc, job.sym[0], 1, 128))
    for name, b, c, sym, heads, hd in cases:
        blob = oracle.encode_blob(b, c, heads, hd, np.array(BINS, np.int32), model)
        table = stream_table(oracle, blob)
        G = sym.shape[2] // 64
        assert len(table) == 2 * G
        total = 0
        for pg, (_, hb, nw, _) in enumerate(table):
            tr = oracle.trace_group_words(np.ascontiguousarray(sym[pg // G]), pg % G, BINS[pg // G], model)
            assert tr.shape == (T,) and tr.max(initial=0) <= 64
            assert int(tr.sum()) == nw, (name, pg)
            assert oracle.stream_head(blob, pg)[2] == hb
            total += nw
        assert name == "patterned" or T == 1 or total > 0


def test_oracle_front_end_takes_a_slice_of_a_job(oracle):
    """Job.refs hands the oracle token slices of the job's KV, which are not contiguous: the ctypes front-end copies them,
    and the copy has to live until the C call returns.  (It did not: the pointer was taken from a temporary, and the first
    run of this file got a blob of freed memory one time in five -- 449 words where the trace said 512.)"""
    job = pattern_job(*PATTERN_JOBS[0])
    bits, code = oracle.torch_to_bits(job.kv().reshape(1, 2, job.n * job.T, job.C))
    part = bits[:, :, job.T:2 * job.T]
    assert not part.flags["C_CONTIGUOUS"]
    want = oracle.encode_blob(np.ascontiguousarray(part), code, job.H, D, np.array(BINS, np.int32))
    for _ in range(8):
        assert oracle.encode_blob(part, code, job.H, D, np.array(BINS, np.int32)) == want
        sym, _ = oracle.quantize(part, code, np.array(BINS, np.int32))
        assert np.array_equal(sym, job.sym[1])
        assert np.array_equal(oracle.trace_group_words(np.asfortranarray(job.sym[1, 0]), 0, BINS[0]), job.words(oracle, 1, 0, 0))


@pytest.mark.parametrize("T,C,dtype", PATTERN_JOBS, ids=PATTERN_IDS)
def test_burst_and_silence_preconditions(oracle, T, C, dtype):
    """What the patterns are FOR, asserted from the trace and the oracle's blobs (conditions of the generator, not
    measurements of a kernel).  Every burst stream has tokens that take all 64 words; the runs at start and middle lie at
    8 distinct values of e mod 128 per plane; and
      T = 256   32-bin plane: a run of >= 16 tokens in which every second token takes 64 words (its 30 once-only symbols
                cost 8 bits each); 16-bin plane: all 14 tokens of its run (a channel has no more once-only symbols)
      T = 2048  two consecutive tokens take 64 words each, and some three tokens take >= 128
    Silent streams have no words in the oracle's blob."""
    job = pattern_job(T, C, dtype)
    tables = [stream_table(oracle, b) for b in job.refs()]
    G = job.G
    offsets = {}
    figures = {"streams": len(job.streams), "burst": 0, "silence": 0}
    for (i, p, g), (family, tag, *off) in sorted(job.streams.items()):
        nw = tables[i][p * G + g][2]
        figures[family] += 1
        if family == "silence":
            assert nw == 0, (job.name, i, p, g, tag)
            continue
        tr = job.words(oracle, i, p, g)
        assert int(tr.sum()) == nw
        if T == 1:
            assert nw == 0
            continue
        assert tr.max() == 64, (job.name, tag)
        if tag.startswith("run at"):
            where = tag.split()[2]
            if where != "end":
                a = int(tag.split("token ")[1].split(")")[0])
                e = int(tr[a + BINS[p] - 2:].sum()) % 128
                assert e == off[0]
                offsets.setdefault((p, where), set()).add(e)
            if T == 256:
                assert longest_alternation(tr) >= (16 if BINS[p] == 32 else 14), (tag, tr.tolist())
                figures[f"alternation, {BINS[p]} bins"] = max(figures.get(f"alternation, {BINS[p]} bins", 0), longest_alternation(tr))
            if T == 2048:
                assert has_pair(tr) and window3(tr) >= 128, (tag, tr.tolist())
                figures["three-token window"] = max(figures.get("three-token window", 0), window3(tr))
    if T > 1:
        assert set(offsets) == {(p, w) for p in (0, 1) for w in ("start", "middle")}
        for key, offs in offsets.items():
            assert len(offs) >= 8, (key, offs)
        figures["offsets e mod 128"] = {f"{BINS[p]} bins, {w}": sorted(o) for (p, w), o in offsets.items()}
    print(f"\n[{job.name}] {job.n} chunks, {2 * G * job.n} streams in the launch; under test: {figures}")


def test_tail_sweep_covers_every_word_count_and_every_grid_pair(oracle):
    """Coverage of the tail sweep, from the directories of the oracle's blobs: every value of nwords mod 128 occurs, and all
    256 pairs of (stream start mod 256) / 16 and (end of the stream's last state word mod 256) / 16.  No pair is excused."""
    jobs = [tail_job(*j) for j in TAIL_JOBS]
    mods, pairs, nstreams = tail_coverage(oracle, jobs)
    print(f"\n[tails] {nstreams} streams in {len(jobs)} jobs of {TAIL_CHUNKS} chunks: {len(mods)} of 128 word counts mod 128, "
          f"{len(pairs)} of 256 (start, end) pairs")
    assert mods == set(range(128)), sorted(set(range(128)) - mods)
    assert pairs == {(s, e) for s in range(16) for e in range(16)}, sorted({(s, e) for s in range(16) for e in range(16)} - pairs)
    silent = sum(1 for job in jobs for b in job.refs() for row in stream_table(oracle, b) if row[2] == 0)
    assert silent >= len(jobs)  # (0 busy lanes comes round in every job: a stream of head + states)


# ---------------------------------------------------------------------------------------------------------------
# 4. the GPU
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nat():
    from lmcache_amd import native
    native.lib()
    return native


@pytest.fixture(scope="module")
def ctx(nat):
    return nat.get_context(0)


def bits_np(t):
    return t.contiguous().cpu().view(torch.int16).numpy().view(np.uint16)


def encode_with_path(nat, ctx, path, kv_dev, n, T, stride):
    """lmc_encode_chunks of n chunks of T tokens under a launch path -> (the blobs' bytes, the device arena)."""
    arena = torch.zeros(n * stride, dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(n, dtype=torch.int32, device=DEV)
    assert arena.data_ptr() % 256 == 0  # the 256-byte grid of tail_coverage is the arena's
    ctx.set_encode_path(path)
    try:
        ctx.encode_chunks(nat.KVLayout.from_chunk(kv_dev, "vllm"), 0, n * T, T, list(BINS), arena.data_ptr(), stride, sizes.data_ptr())
        torch.cuda.synchronize()
    finally:
        ctx.set_encode_path("auto")
    assert ctx.status(clear=True) == 0, f"{path}: encode status"
    sz = sizes.cpu().tolist()
    host = arena.cpu().numpy()
    return [host[i * stride:i * stride + sz[i]].tobytes() for i in range(n)], arena


def upload(blobs, stride):
    host = np.zeros(len(blobs) * stride, np.uint8)
    for i, b in enumerate(blobs):
        host[i * stride:i * stride + len(b)] = np.frombuffer(b, np.uint8)
    return torch.from_numpy(host).to(DEV)


def check_decodes(nat, ctx, job, arena, stride, want_sym, want_bf, want_fp, full=True):
    """Every way out of the decoder for the n blobs in `arena`: symbols, contiguous bf16 (the eight-token block path),
    fp16 (the one-token path), two paged destinations (block-ordered and token-random slots), a negative first
    destination token with 3 tokens skipped.  Bit-equal to the oracle's decode, status 0."""
    n, T, H, C = job.n, job.T, job.H, job.C
    ntok = n * T

    def done(what):
        torch.cuda.synchronize()
        assert ctx.status(clear=True) == 0, f"{job.name}: {what}: decode status"

    sym = torch.cat([ctx.decode_symbols(arena[i * stride:], 1, H, D, T) for i in range(n)], dim=1)
    done("symbols")
    assert np.array_equal(sym.cpu().numpy(), want_sym), f"{job.name}: decode_symbols"
    for odt, want in ((torch.bfloat16, want_bf), (torch.float16, want_fp)):
        out = torch.zeros(1, 2, ntok, H, D, dtype=odt, device=DEV)
        ctx.decode_chunks(arena.data_ptr(), stride, n, nat.KVLayout.from_chunk(out, "vllm"), 0, T)
        done(str(odt))
        assert np.array_equal(bits_np(out).reshape(1, 2, ntok, C), want), f"{job.name}: contiguous {odt}"
    if not full:
        return
    g = torch.Generator().manual_seed(ntok)
    bs, first = 16, 5
    nb = (first + ntok + bs - 1) // bs + 3
    pos = torch.arange(first, first + ntok)
    ordered = torch.randperm(nb, generator=g)[pos // bs] * bs + pos % bs
    scattered = torch.randperm(nb * bs, generator=g)[:ntok]
    for what, slots, layout in (("block-ordered slots", ordered, "NBHD"), ("token-random slots", scattered, "NHBD")):
        cache = torch.zeros((2, nb, bs, H, D) if layout == "NBHD" else (2, nb, H, bs, D), dtype=torch.bfloat16, device=DEV)
        ctx.decode_chunks(arena.data_ptr(), stride, n, nat.KVLayout.paged([cache], slots, bs, layout), 0, T)
        done(what)
        c = cache.cpu()
        flat = c.reshape(2, nb * bs, H, D) if layout == "NBHD" else c.permute(0, 1, 3, 2, 4).reshape(2, nb * bs, H, D)
        assert np.array_equal(bits_np(flat[:, slots]).reshape(2, ntok, C), want_bf[0]), f"{job.name}: {what}"
        untouched = torch.ones(nb * bs, dtype=torch.bool)
        untouched[slots] = False
        assert not bits_np(flat[:, untouched]).any(), f"{job.name}: {what}: written outside the slot mapping"
    skip = 3
    if ntok > skip:
        out = torch.zeros(1, 2, ntok - skip, H, D, dtype=torch.bfloat16, device=DEV)
        ctx.decode_chunks(arena.data_ptr(), stride, n, nat.KVLayout.from_chunk(out, "vllm"), -skip, T)
        done("skip")
        assert np.array_equal(bits_np(out).reshape(1, 2, ntok - skip, C), want_bf[:, :, skip:]), f"{job.name}: first tokens skipped"


def run_job(nat, ctx, oracle, job):
    refs = job.refs()
    stride = nat.r16(nat.blob_bound(1, job.T, job.H, D))
    assert stride == job.stride(oracle)
    assert np.array_equal(np.concatenate([oracle.decode_blob_symbols(b) for b in refs], axis=1), job.table())
    kv_dev = job.kv().to(DEV)
    arena = None
    for path in ("two_kernels", "fused"):
        blobs, arena = encode_with_path(nat, ctx, path, kv_dev, job.n, job.T, stride)
        for i, (got, ref) in enumerate(zip(blobs, refs)):
            assert len(got) == len(ref) and got == ref, f"{job.name}: {path}, chunk {i} of {job.n} differs from the oracle's blob"
    check_decodes(nat, ctx, job, arena, stride, job.table(), job.want(oracle.BF16), job.want(oracle.FP16))


@gpu
@pytest.mark.parametrize("T,C,dtype", PATTERN_JOBS, ids=PATTERN_IDS)
def test_bursts_and_silence_on_the_gpu(nat, ctx, oracle, T, C, dtype):
    """The lockstep runs and the silent streams through both encode launch paths and every decode path.  This is the
    test that holds the decoder's every-second-token ring check (k_decode.h: a token takes at most 64 words and a whole
    block lies below the upper one) and the encoder's every-second-token flush test against streams that take 64 words
    at consecutive tokens."""
    run_job(nat, ctx, oracle, pattern_job(T, C, dtype))


@gpu
@pytest.mark.parametrize("T,C,dtype", TAIL_JOBS, ids=TAIL_IDS)
def test_tail_sweep_on_the_gpu(nat, ctx, oracle, T, C, dtype):
    """Every word count mod 128 and every (start, end) pair on the 256-byte grid (coverage:
    test_tail_sweep_covers_every_word_count_and_every_grid_pair, asserted again here over the jobs) through both encode
    paths and every decode path."""
    mods, pairs, _ = tail_coverage(oracle, [tail_job(*j) for j in TAIL_JOBS])
    assert len(mods) == 128 and len(pairs) == 256
    run_job(nat, ctx, oracle, tail_job(T, C, dtype))


@gpu
@pytest.mark.parametrize("T,C,dtype", [j for j in PATTERN_JOBS if 1 < j[0] <= 256], ids=[i for i, j in zip(PATTERN_IDS, PATTERN_JOBS) if 1 < j[0] <= 256])
def test_cdf16_blobs_of_the_short_patterns_still_decode(nat, ctx, oracle, T, C, dtype):
    """What rounds 3-4 wrote for chunks of up to 256 tokens: the same patterns as CDF16 blobs (the oracle's, uploaded).  A
    lockstep run costs 11 bits a token there, so 64-word tokens follow each other more closely than in the counts model."""
    job = pattern_job(T, C, dtype)
    old = job.refs(oracle.MODEL_CDF16)
    assert all(oracle.parse_header(b)["model"] == oracle.MODEL_CDF16 for b in old)
    stride = nat.r16(nat.blob_bound(1, T, job.H, D))
    check_decodes(nat, ctx, job, upload(old, stride), stride, job.table(), job.want(oracle.BF16, oracle.MODEL_CDF16),
                  job.want(oracle.FP16, oracle.MODEL_CDF16))


@gpu
def test_e4m3_patterns_through_the_fused_path(nat, ctx, oracle):
    """The fp8 encoders are kernel instances of their own: the T = 256, C = 384 patterns as float8_e4m3fn KV (integers up
    to 15 are exact there) through the fused path.  The blob is the oracle's blob of the bf16 images with header word 23
    set to the fp8 code (include/lmc_format.h)."""
    job = pattern_job(256, 384, torch.float16)
    kv = job.kv(torch.float8_e4m3fn)
    bits, code = oracle.torch_to_bits(kv.to(torch.bfloat16).reshape(1, 2, job.n * job.T, job.C))
    word23 = struct.pack("<I", nat.dtype_code(torch.float8_e4m3fn))
    refs = []
    for i in range(job.n):
        b = oracle.encode_blob(bits[:, :, i * job.T:(i + 1) * job.T], code, job.H, D, np.array(BINS, np.int32))
        refs.append(b[:92] + word23 + b[96:])
    stride = nat.r16(nat.blob_bound(1, job.T, job.H, D))
    blobs, arena = encode_with_path(nat, ctx, "fused", kv.to(DEV), job.n, job.T, stride)
    for i, (got, ref) in enumerate(zip(blobs, refs)):
        assert got == ref, f"chunk {i}"
    want = lambda c: np.concatenate([oracle.decode_blob(b, c) for b in refs], axis=2)
    check_decodes(nat, ctx, job, arena, stride, job.table(), want(oracle.BF16), want(oracle.FP16), full=False)


@gpu
def test_pack_of_silent_and_burst_streams(nat, oracle):
    """store_pack / finish_pack / load_pack through the codec on the T = 256, C = 128 patterns: the pack holds silent and
    burst streams side by side -- segments whose streams have no words in k_pack_scan and k_pack_copy -- and is the oracle's
    pack_from_blobs byte for byte (test_gpu_codec.py's _pack_case: pack bytes, extraction, three loads)."""
    from lmcache_amd.storage_backend.serde.cachegen_device import CacheGenDeviceCodec, PinnedArena
    from tests.test_gpu_codec import _pack_case
    job = pattern_job(256, 128, torch.bfloat16)
    tables = [stream_table(oracle, b) for b in job.refs()]
    assert any(all(row[2] == 0 for row in t[:job.G]) for t in tables), "no plane segment made of silent streams alone"
    x = job.kv().reshape(1, 2, job.n * job.T, job.C)
    codec, arena = CacheGenDeviceCodec(0), PinnedArena()
    try:
        codec.pack_parts = 1  # (2 planes: the store is one part)
        pack, blobs = _pack_case(oracle, codec, arena, job.name, x, job.H, D, job.T, list(BINS), "fused", False)
        assert blobs == job.refs()
    finally:
        arena.close()
        codec.close()
