"""Input domains and plain references for the device arithmetic tests (tests/test_gpu_device_arith.py on the GPU,
tests/test_device_arith_host.py for what holds without one).  Everything here is numpy / torch-CPU / integer
arithmetic written from the operations' definitions: none of it is shared with, or derived from, the device helpers."""
import numpy as np
import torch

BF16, FP16 = 0, 1
DTYPES = {"bf16": BF16, "fp16": FP16}
MAXES = range(1, 16)  # MAX = bins // 2 - 1 of the bin counts 4 .. 33
CDF_SCALE = 65504     # 2^16 - 32


def widen(bits, dtype: int) -> np.ndarray:
    """16-bit patterns -> their values as fp32 (exact for both dtypes); fp16 through torch's CPU cast."""
    bits = np.ascontiguousarray(bits, dtype=np.uint16)
    if dtype == BF16:
        return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return torch.from_numpy(bits.view(np.int16)).view(torch.float16).to(torch.float32).numpy()


def f32_bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_floats(got_bits, want_bits) -> np.ndarray:
    """Bit equality of fp32 patterns, any NaN equal to any NaN."""
    g, w = np.asarray(got_bits, np.uint32), np.asarray(want_bits, np.uint32)
    return (g == w) | (np.isnan(g.view(np.float32)) & np.isnan(w.view(np.float32)))


# ---- (a) the row factor -------------------------------------------------------------------------------------------------
def row_in_range(bits, dtype: int) -> np.ndarray:
    """The rule lmc_device.h states for the short division: bf16 maxes with a biased exponent of 27 .. 227, fp16 maxes
    that are finite and not zero."""
    bits = np.asarray(bits, np.uint32)
    if dtype == BF16:
        e = (bits >> 7) & 0xff
        return (e >= 27) & (e <= 227)
    return (bits != 0) & (bits < 0x7c00)


def row_factor(max_bits, MAX, dtype: int) -> np.ndarray:
    """MAX / max in IEEE fp32 (zero -> inf, inf -> 0, NaN -> NaN, denormal quotients kept)."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        return (np.asarray(MAX, np.float32) / widen(max_bits, dtype)).astype(np.float32)


# ---- (b), (c) the quantise step -----------------------------------------------------------------------------------------
SEED_ROWS = 1  # default_rng(SEED_ROWS): the 64 in-range maxes per dtype


def seeded_maxes(dtype: int) -> np.ndarray:
    """64 row maxes inside the short division's range, uniform over its bit patterns."""
    rng = np.random.default_rng(SEED_ROWS)
    bf = rng.integers(27 << 7, 228 << 7, 64)
    fp = rng.integers(1, 0x7c00, 64)
    return (bf if dtype == BF16 else fp).astype(np.uint16)


def edge_maxes(dtype: int) -> np.ndarray:
    """The first and last patterns of the range (bf16: exponents 27 and 227 with mantissa 0 and 0x7f)."""
    if dtype == BF16:
        return np.array([27 << 7, (27 << 7) | 0x7f, 227 << 7, (227 << 7) | 0x7f], np.uint16)
    return np.array([0x0001, 0x03ff, 0x0400, 0x7bff], np.uint16)


def outside_maxes(dtype: int) -> np.ndarray:
    """Finite non-zero maxes outside the range: rows every quantiser but the fused one's short division still takes
    through the regular step (bf16: the neighbours of the range, the smallest normal, the largest finite, the largest
    denormal -- regular for the MAX whose factor stays finite)."""
    if dtype == BF16:
        return np.array([(26 << 7) | 0x7f, 228 << 7, 1 << 7, 0x7f7f, 0x007f], np.uint16)
    return np.array([], np.uint16)


def row_x_bits(max_bits: int) -> np.ndarray:
    """Every finite pattern x with |x| <= max: 0 .. max and their negatives."""
    m = np.arange(int(max_bits) + 1, dtype=np.uint16)
    return np.concatenate([m, m | np.uint16(0x8000)])


class QuantDomain:
    """Rows (maxes) and, concatenated, every x of every row: x_bits, x (fp32), row (index into maxes)."""

    def __init__(self, dtype: int, maxes):
        self.dtype, self.maxes = dtype, np.asarray(maxes, np.uint16)
        xs = [row_x_bits(m) for m in self.maxes]
        self.x_bits = np.concatenate(xs)
        self.row = np.repeat(np.arange(len(xs), dtype=np.uint32), [len(v) for v in xs])
        if len(self.x_bits) & 1:  # the pair kernel takes an even count: the last case once more
            self.x_bits, self.row = np.append(self.x_bits, self.x_bits[-1]), np.append(self.row, self.row[-1])
        self.x = widen(self.x_bits, dtype)

    def factors(self, MAX: int) -> np.ndarray:
        return row_factor(self.maxes, MAX, self.dtype)


def quant_ref(x, factor, MAX) -> np.ndarray:
    """round(x * factor + MAX) with the product and the sum each rounded to fp32, ties to even; as fp32."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        y = (np.asarray(x, np.float32) * np.asarray(factor, np.float32)).astype(np.float32)
        return np.rint((y + np.float32(MAX)).astype(np.float32))


def quant_single_rounding(x, factor, MAX) -> np.ndarray:
    """What a fused multiply-add would give: x * factor is exact in float64 (at most 35 significant bits), the sum is
    rounded once."""
    z = np.asarray(x, np.float64) * np.asarray(factor, np.float64) + np.float64(MAX)
    return np.rint(z.astype(np.float32))


def quant_special_ref(x, factor, MAX) -> np.ndarray:
    """The special rows' rule (k_quantize.h): r = the regular step's rounded value; NaN and |r| >= 2^31 give 0 (the low
    byte of INT_MIN, what the CPU's float -> int8 conversion leaves), anything else the low byte of the integer r."""
    r = quant_ref(x, factor, MAX)
    ok = np.abs(r) < np.float32(2147483648.0)  # False for NaN
    # (the inner where keeps NaN and the huge values out of the integer cast)
    return np.where(ok, np.where(ok, r, 0).astype(np.int64) & 0xff, 0).astype(np.uint32)


def sensitivity(dom: QuantDomain):
    """(elements whose symbol changes under a single-rounding evaluation, elements whose symbol changes when the factor
    is one ulp larger) over the domain, MAX 1 .. 15."""
    fused = ulp = 0
    for MAX in MAXES:
        f = dom.factors(MAX)[dom.row]
        ref = quant_ref(dom.x, f, MAX)
        fused += int(np.count_nonzero(quant_single_rounding(dom.x, f, MAX) != ref))
        ulp += int(np.count_nonzero(quant_ref(dom.x, np.nextafter(f, np.float32(np.inf)), MAX) != ref))
    return fused, ulp


def special_rows(dtype: int):
    """(max pattern, MAX) pairs the quantisers treat as special: the factor or the max is not finite.  Zero, inf and NaN
    maxes, and for bf16 the denormal maxes whose factor overflows."""
    if dtype == BF16:
        maxes = [0x0000, 0x0001, 0x0002, 0x0040, 0x007f, 0x7f80, 0x7f81, 0x7fc0, 0x7fff]
    else:
        maxes = [0x0000, 0x7c00, 0x7c01, 0x7e00, 0x7fff]
    rows = []
    for m in maxes:
        for MAX in MAXES:
            f = row_factor(np.array([m], np.uint16), MAX, dtype)[0]
            if not np.isfinite(f) or not np.isfinite(widen(np.array([m], np.uint16), dtype)[0]):
                rows.append((m, MAX))
    return rows


# ---- (d) the coder's division -------------------------------------------------------------------------------------------
def rans_cases(seed: int = 2):
    """(x, f, st) as uint32: every f in 1 .. 65535; x at the quotient steps q f - 1, q f, q f + 1 of chosen and seeded q,
    at the domain's ends and at seeded places, all below f * 2^16; st in {0, 2^16 - f, seeded in between}."""
    rng = np.random.default_rng(seed)
    f = np.arange(1, 65536, dtype=np.int64)
    qfix = np.unique([1, 2, 3, 65535] + [(1 << k) + d for k in range(2, 16) for d in (-1, 0, 1)])
    q = np.concatenate([np.broadcast_to(qfix, (len(f), len(qfix))), rng.integers(0, 65536, (len(f), 64))], axis=1)
    steps = (q * f[:, None])[:, :, None] + np.array([-1, 0, 1])
    lim = f << 16
    ends = np.stack([lim - 1, np.full_like(f, 65536), np.zeros_like(f)], axis=1)
    spread = rng.integers(0, lim[:, None], (len(f), 64))
    x = np.concatenate([steps.reshape(len(f), -1), ends, spread], axis=1)
    ff = np.broadcast_to(f[:, None], x.shape)
    keep = (x >= 0) & (x < lim[:, None])
    x, ff = x[keep], ff[keep]
    c = 65536 - ff
    kind = np.arange(len(x)) % 3
    st = np.where(kind == 0, 0, np.where(kind == 1, c, rng.integers(0, 65536, len(x)) % (c + 1)))
    return x.astype(np.uint32), ff.astype(np.uint32), st.astype(np.uint32)


def rans_ref(x, f, st):
    x, f, st = (np.asarray(a, np.uint64) for a in (x, f, st))
    q, r = x // f, x % f
    return q.astype(np.uint32), r.astype(np.uint32), (((q << np.uint64(16)) + r + st) & np.uint64(0xffffffff)).astype(np.uint32)


# ---- (e) the CDF arithmetic ---------------------------------------------------------------------------------------------
def rne_cases(seed: int = 3, exhaustive_below: int = 1024):
    """(n, T) as int64: every T in 1 .. 65535 with n in {0, 1, T/2 - 1 .. T/2 + 1, T - 1, T} and 64 seeded n <= T; every
    n for T <= exhaustive_below."""
    rng = np.random.default_rng(seed)
    T = np.arange(1, 65536, dtype=np.int64)
    h = T // 2
    fixed = np.stack([np.zeros_like(T), np.ones_like(T), h - 1, h, h + 1, T - 1, T], axis=1)
    n = np.concatenate([np.clip(fixed, 0, T[:, None]), rng.integers(0, T[:, None] + 1, (len(T), 64))], axis=1)
    TT = np.broadcast_to(T[:, None], n.shape)
    ns, Ts = [n.ravel()], [TT.ravel()]
    for t in range(1, exhaustive_below + 1):
        ns.append(np.arange(t + 1, dtype=np.int64))
        Ts.append(np.full(t + 1, t, np.int64))
    return np.concatenate(ns), np.concatenate(Ts)


def rne_ref(v, T):
    """(RNE(v / T), whether v / T lies exactly between two integers) in integers."""
    v, T = np.asarray(v, np.int64), np.asarray(T, np.int64)
    q, r = v // T, v % T
    tie = 2 * r == T
    return q + ((2 * r > T) | (tie & (q & 1 == 1))), tie


def rne_magic(T) -> np.ndarray:
    """floor(2^32 / T), 0xffffffff for T = 1: the reciprocal the CDF code hands to rne_div_u32."""
    T = np.asarray(T, np.int64)
    return np.where(T == 1, 0xffffffff, (1 << 32) // T)


def rne_emulated(v, T):
    """rne_div_u32 in integers -> (result, corrections the estimate needed).  The device has two correction steps."""
    v, T = np.asarray(v, np.int64), np.asarray(T, np.int64)
    q = (v * rne_magic(T)) >> 32
    r = v - q * T
    need = r // T
    q, r = q + need, r - need * T
    return q + ((2 * r > T) | ((2 * r == T) & (q & 1 == 1))), need


CDF_T = (1, 2, 3, 255, 256, 257, 300, 768, 1000, 4096, 32768, 65535)
CDF_NSYM = (2, 3, 15, 16, 17, 30, 31)


def cdf_cases(seed: int = 4, wide: bool = False):
    """Histograms per (T, nsym): counts [case][64 lanes][32 symbols] that sum to T over the symbols below nsym.  Lane 0:
    all in symbol 0; lane 1: all in the last symbol; lane 2: a column of ones (what is left of T in a seeded symbol);
    the others seeded, half of them peaked."""
    rng = np.random.default_rng(seed)
    Ts, ns, counts = [], [], []
    for T in CDF_T:
        for nsym in CDF_NSYM:
            if wide and nsym > 16:
                continue
            c = np.zeros((64, 32), np.int64)
            c[0, 0] = T
            c[1, nsym - 1] = T
            ones = min(T, nsym)
            c[2, :ones] = 1
            c[2, rng.integers(0, nsym)] += T - ones
            for lane in range(3, 64):
                p = rng.dirichlet(np.full(nsym, 0.3 if lane & 1 else 3.0))
                c[lane, :nsym] = rng.multinomial(T, p)
            assert (c.sum(axis=1) == T).all()
            Ts.append(T), ns.append(nsym), counts.append(c)
    return np.array(counts), np.array(Ts, np.int64), np.array(ns, np.int64)


def cdf_ref(counts, T, nsym) -> np.ndarray:
    """cdf[i] = RNE(N_i * 65504 / T) + i for i = 0 .. 32, N_i = the number of symbols below i -- T from entry nsym on,
    since the symbols are 0 .. nsym - 1.  [case][lane][33], not yet reduced to 16 bits (entry 32 is 65536)."""
    counts = np.asarray(counts, np.int64)
    T, nsym = np.asarray(T, np.int64)[:, None, None], np.asarray(nsym, np.int64)[:, None, None]
    N = np.concatenate([np.zeros(counts.shape[:2] + (1,), np.int64), np.cumsum(counts, axis=2)], axis=2)
    i = np.arange(33)[None, None, :]
    N = np.where(i >= nsym, T, N)
    return rne_ref(N * CDF_SCALE, T)[0] + i


def pack_hreg(counts) -> np.ndarray:
    """counts [case][lane][32] -> the kernels' registers [case][16][lane]: count of symbol 2k | count of 2k + 1 << 16."""
    c = np.asarray(counts, np.uint32)
    return np.ascontiguousarray((c[:, :, 0::2] | (c[:, :, 1::2] << np.uint32(16))).transpose(0, 2, 1))


def cdf_wide_ref(cdf) -> np.ndarray:
    """The decoder's packed form of entries 0 .. 15: cdf[i] << 16 | (cdf[i + 1] - cdf[i]), at [i / 4][lane][i % 4]."""
    e = ((cdf[:, :, :16] << 16) | (cdf[:, :, 1:17] - cdf[:, :, :16])).astype(np.uint32)  # [case][lane][16]
    return np.ascontiguousarray(e.reshape(e.shape[0], 64, 4, 4).transpose(0, 2, 1, 3))


def golden_cdf_cases(z, T: int):
    """The fixture's symbols of chunk length T as histogram cases: (counts [case][64][32], nsym [case], the fixture's CDF
    [case][64][33], which lanes are real).  96 channels per plane: a full wave and a half one; a plane's nsym is its
    largest symbol + 1."""
    sym, want = z[f"T{T}_sym"].astype(np.int64), z[f"T{T}_cdf"].astype(np.int64)  # [2][T][96], [2][96][33]
    counts, cdfs, real, nsym = [], [], [], []
    for p in range(sym.shape[0]):
        hist = np.stack([(sym[p] == s).sum(axis=0) for s in range(32)], axis=1)  # [96][32]
        for c0 in (0, 64):
            c = np.zeros((64, 32), np.int64)
            w = np.zeros((64, 33), np.int64)
            k = min(64, hist.shape[0] - c0)
            c[:k], w[:k] = hist[c0:c0 + k], want[p, c0:c0 + k]
            counts.append(c), cdfs.append(w), real.append(np.arange(64) < k), nsym.append(max(int(sym[p].max()) + 1, 2))
    return np.array(counts), np.array(nsym, np.int64), np.array(cdfs), np.array(real)


# ---- (f) small exact pieces -----------------------------------------------------------------------------------------------
def divmod_small_cases():
    """divmod_small's stated domain: R 2 .. 30, e < 2^15."""
    R = np.repeat(np.arange(2, 31, dtype=np.uint32), 1 << 15)
    return np.tile(np.arange(1 << 15, dtype=np.uint32), 29), R


def split_divmod_cases():
    """split_divmod's stated domain: R 4 .. 2048, e < 2048."""
    R = np.repeat(np.arange(4, 2049, dtype=np.uint32), 2048)
    return np.tile(np.arange(2048, dtype=np.uint32), 2045), R


def float_divmod(e, R):
    """The one-multiply division as a numpy statement: trunc((e + 0.5) * fl(1 / R)) in fp32."""
    rcp = (np.float32(1.0) / R.astype(np.float32)).astype(np.float32)
    q = ((e.astype(np.float32) + np.float32(0.5)) * rcp).astype(np.float32).astype(np.uint32)
    return q, e - q * R, rcp


def f2bf16_inputs() -> np.ndarray:
    """fp32 patterns (h << 16) + {0, 1, 0x7fff, 0x8000, 0x8001, 0xffff} for every 16-bit h: exact values, both sides of
    every midpoint and the midpoints, NaN payloads, infinities, zeros, denormals."""
    h = np.arange(1 << 16, dtype=np.uint32) << np.uint32(16)
    return (h[:, None] + np.array([0, 1, 0x7fff, 0x8000, 0x8001, 0xffff], np.uint32)).ravel()


def f2bf16_ref(fbits) -> np.ndarray:
    t = torch.from_numpy(np.ascontiguousarray(fbits, np.uint32).view(np.int32)).view(torch.float32)
    return t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).astype(np.uint32)


def f2fp16_inputs() -> np.ndarray:
    """fp32 patterns: every fp16 value, the midpoint to its successor and one fp32 ulp either side of it (both signs);
    65504 .. 65536 in fp32 ulps around 65520 (where the cast turns to inf); fp32 denormals; NaNs."""
    hb = np.arange(0x7c01, dtype=np.uint16)  # 0 .. inf
    v = widen(hb, FP16).astype(np.float64)
    mid = ((v[:-1] + v[1:]) / 2).astype(np.float32)  # exact: a 12-bit significand, no smaller than 2^-25
    assert np.array_equal(mid.astype(np.float64), (v[:-1] + v[1:]) / 2)
    mb = f32_bits(mid)
    pos = np.concatenate([f32_bits(v.astype(np.float32)), mb, mb - 1, mb + 1])
    top = f32_bits(np.array([65520.0], np.float32))[0]
    lo, hi = f32_bits(np.array([65504.0, 65536.0], np.float32))
    pos = np.concatenate([pos, np.arange(top - 64, top + 65, dtype=np.uint32), np.array([lo, lo + 1, hi - 1, hi, hi + 1], np.uint32),
                          np.array([1, 2, 0x007fffff, 0x00400000, 0x00800000], np.uint32),
                          np.array([0x7f800001, 0x7fc00000, 0x7fffffff, 0x7f800000, 0x7f7fffff], np.uint32)])
    return np.concatenate([pos, pos | np.uint32(0x80000000)])


def f2fp16_ref(fbits) -> np.ndarray:
    t = torch.from_numpy(np.ascontiguousarray(fbits, np.uint32).view(np.int32)).view(torch.float32)
    return t.to(torch.float16).view(torch.int16).numpy().view(np.uint16).astype(np.uint32)


def transpose_cases(seed: int = 5) -> np.ndarray:
    """[case][64] uint64 rows: every single-bit matrix, the identity, all ones, 256 seeded matrices."""
    rng = np.random.default_rng(seed)
    single = np.zeros((4096, 64), np.uint64)
    rc = np.arange(4096)
    single[rc, rc >> 6] = np.uint64(1) << (rc & 63).astype(np.uint64)
    ident = (np.uint64(1) << np.arange(64, dtype=np.uint64))[None, :]
    ones = np.full((1, 64), 0xffffffffffffffff, np.uint64)
    rand = rng.integers(0, 1 << 64, (256, 64), dtype=np.uint64)
    return np.concatenate([single, ident, ones, rand])


def transpose_ref(rows) -> np.ndarray:
    """out[case][k] bit l = rows[case][l] bit k."""
    k = np.arange(64, dtype=np.uint64)
    bits = (rows[:, :, None] >> k[None, None, :]) & np.uint64(1)  # [case][l][k]
    return (bits << k[None, :, None]).sum(axis=1, dtype=np.uint64)  # (disjoint bits: the sum is the OR)


# ---- the end-to-end leg: rows for the encoders that sit on the quantise step's decision points ------------------------
E2E_L, E2E_H, E2E_D, E2E_CHUNK, E2E_NCHUNKS = 8, 2, 64, 256, 3
E2E_BINS = list(range(4, 33, 2)) + [23]  # every MAX 1 .. 15, and one odd bin count


def e2e_planted(dtype: int) -> np.ndarray:
    """Row maxes planted at every token position mod 8: the range's edge patterns, their neighbours outside it, zero, the
    smallest denormal, the largest finite value, inf and NaN."""
    if dtype == BF16:
        return np.concatenate([edge_maxes(BF16), np.array([(26 << 7) | 0x7f, 228 << 7, 0x0000, 0x0001, 0x7f7f, 0x7f80, 0x7fc0], np.uint16)])
    return np.concatenate([edge_maxes(FP16), np.array([0x0000, 0x7c00, 0x7e00], np.uint16)])  # (0x0001 and 0x7bff are edges)


def _is_regular(m: int, MAX: int, dtype: int) -> bool:
    one = np.array([m], np.uint16)
    return m != 0 and bool(np.isfinite(widen(one, dtype)[0])) and bool(np.isfinite(row_factor(one, MAX, dtype)[0]))


def _e2e_row(m: int, MAX: int, dtype: int, C: int, rng) -> np.ndarray:
    """One row of C channels with max pattern m.  Regular: the max, then the C - 1 magnitudes <= max whose
    fl(x * factor) + MAX lies nearest a half-integer, signs alternating.  Special: seeded magnitudes <= m, m among them."""
    if not _is_regular(m, MAX, dtype):
        row = rng.integers(0, m + 1, C).astype(np.uint16)
        row[rng.integers(0, C)] = m
        return row | (rng.integers(0, 2, C).astype(np.uint16) << np.uint16(15))
    cand = np.arange(m + 1, dtype=np.uint16)
    f = row_factor(np.array([m], np.uint16), MAX, dtype)[0]
    with np.errstate(under="ignore"):
        z = (widen(cand, dtype) * f).astype(np.float32).astype(np.float64) + MAX
    d = np.abs(z - np.floor(z) - 0.5)
    pick = np.sort(np.argsort(d, kind="stable")[:C - 1])
    row = np.concatenate([[m], np.resize(cand[pick], C - 1)]).astype(np.uint16)
    row[1::2] |= np.uint16(0x8000)
    return row


def e2e_chunk(dtype: int, seed: int = 6):
    """-> (bits uint16 [L][2][T][C], row max pattern [P][T]) of the end-to-end leg: plane p (K of the layers, then V) is
    coded with E2E_BINS[p]; token 8 * (8 i + j) + j holds planted max i (every planted max at every position mod 8, always
    beside in-range rows in its pair and oct), the others cycle through the seeded maxes."""
    rng = np.random.default_rng(seed)
    L, C, T = E2E_L, E2E_H * E2E_D, E2E_CHUNK * E2E_NCHUNKS
    planted, cyc = e2e_planted(dtype), seeded_maxes(dtype)
    assert 8 * (8 * len(planted) - 1) + 7 < T
    bits, maxes, rows = np.zeros((L, 2, T, C), np.uint16), np.zeros((2 * L, T), np.uint16), {}
    for p in range(2 * L):
        MAX = E2E_BINS[p] // 2 - 1
        m_of = cyc[(np.arange(T) + 5 * p) % 64].copy()
        for i, m in enumerate(planted):
            for j in range(8):
                m_of[8 * (8 * i + j) + j] = m
        for t in range(T):
            key = (int(m_of[t]), MAX)
            if key not in rows:
                rows[key] = _e2e_row(key[0], MAX, dtype, C, rng)
            bits[p % L, p // L, t] = rows[key]
        maxes[p] = m_of
    return bits, maxes


def e2e_ulp_sensitivity(bits, maxes, dtype: int) -> int:
    """Elements of the leg's regular rows whose symbol changes when the row's factor is one ulp larger."""
    L, n = bits.shape[0], 0
    for p in range(2 * L):
        MAX = E2E_BINS[p] // 2 - 1
        x = widen(bits[p % L, p // L].ravel(), dtype).reshape(bits.shape[2], -1)
        f = row_factor(maxes[p], MAX, dtype)
        reg = np.isfinite(f) & np.isfinite(widen(maxes[p], dtype)) & (maxes[p] != 0)
        x, f = x[reg], f[reg][:, None]
        n += int(np.count_nonzero(quant_ref(x, np.nextafter(f, np.float32(np.inf)), MAX) != quant_ref(x, f, MAX)))
    return n
