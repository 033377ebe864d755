"""The device helpers that stand in for a plain operation -- a division by v_rcp_f32 and three more instructions, a
quantise step in packed fp32 with a byte-inserting conversion, quotients from a biased float estimate, RNE(N 65504 / T) by
a multiply-high, casts, a 64 x 64 bit transpose by swizzles -- each over every input it can meet (or the chosen points of
a domain too large for that), bit for bit against the references of tests/arith_cases.py.  The kernels under test are
those of tests/csrc/arith_harness.hip: the product's own functions, compiled with the library's own flags
(tests/arith_harness.py).  Every assertion is exact equality.

Last: one end-to-end leg that puts rows on the quantise step's decision points through the three encoders, so that what
the helpers' tests hold is also what the kernels use."""
import os

import numpy as np
import pytest
import torch

from lmcache_amd import native
from tests import arith_cases as ac
from tests import arith_harness as ah
from tests import fixed_model as fm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_SIGNED = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


@pytest.fixture(scope="module")
def harness():
    """The harness library: built here if need be (a missing library without a compiler is an error, not a skip)."""
    ah.build()
    return ah.lib()


def up(a) -> torch.Tensor:
    """A numpy array on the device (unsigned types travel as their signed twins: the kernels see the same bits)."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_SIGNED.get(a.dtype, a.dtype))).to(DEV)


def out(n, dtype=torch.int32, fill=0x5a5a5a5a) -> torch.Tensor:
    return torch.full((int(n),), fill, dtype=dtype, device=DEV)


def down(t, dtype=np.uint32) -> np.ndarray:
    torch.cuda.synchronize()
    return t.cpu().numpy().view(dtype)


def u32(a) -> np.ndarray:
    return np.ascontiguousarray(a).astype(np.uint32)


# ------------------------------------------------------------------ (a) the row factor
@pytest.mark.parametrize("name", list(ac.DTYPES))
def test_row_factor_every_max_pattern(harness, name):
    """Every pattern 0x0000 .. 0x7fff as a row max x MAX 1 .. 15 (491 520 cases per dtype): row_div_in_range is the
    stated rule; inside it row_div_short has the bits of MAX / max in IEEE fp32; and the division the quantisers fall
    back to has those bits for EVERY pattern -- zero -> inf, denormal quotients, inf and NaN maxes (NaN as NaN)."""
    dt = ac.DTYPES[name]
    bits = np.tile(np.arange(0x8000, dtype=np.uint32), 15)
    MAX = np.repeat(np.arange(1, 16, dtype=np.uint32), 0x8000)
    n = len(bits)
    in_range, short, div = out(n), out(n), out(n)
    ah.call("ah_row_factor", up(bits), up(MAX), dt, in_range, short, div, n=n)
    want = ac.f32_bits(ac.row_factor(bits.astype(np.uint16), MAX, dt))
    rng_want = ac.row_in_range(bits, dt)
    assert np.array_equal(down(in_range), rng_want.astype(np.uint32))
    bad = down(short)[rng_want] != want[rng_want]
    assert not bad.any(), f"row_div_short: {int(bad.sum())} of {int(rng_want.sum())} in-range factors differ from the division"
    outside = ~ac.same_floats(down(short), want) & ~rng_want  # (why the range test exists: not asserted, the range may grow)
    print(f"{name}: outside the range row_div_short differs from the division at {int(outside.sum())} of {int((~rng_want).sum())}")
    bad = ~ac.same_floats(down(div), want)
    assert not bad.any(), f"maxf / sf: {int(bad.sum())} of {n} differ from IEEE fp32 (first: max {bits[bad][0]:#06x}, MAX {MAX[bad][0]})"


# ------------------------------------------------------------------ (b) the quantise step
@pytest.mark.parametrize("name", list(ac.DTYPES))
def test_quantise_step_every_x_of_chosen_rows(harness, name):
    """Rows: the 64 seeded in-range maxes, the range's edge patterns, and finite maxes outside the range (regular rows of
    every quantiser but the fused one's short path); MAX 1 .. 15; every finite x with |x| <= max: 34.5 M (bf16) / 34.3 M
    (fp16) elements.  quant_fast, quant_special's low byte and quant_z2 + v_cvt_pk_u8_f32 at each byte position must all
    be round(fl(fl(x * factor) + MAX)), the conversion leaving the other three bytes of its dword alone.  What makes this
    sharp -- how many of these elements a fused multiply-add or a one-ulp factor error would move -- is held by
    tests/test_device_arith_host.py and asserted again below (bf16 85 / 482, fp16 89 / 463 with these rows; caps 50 / 300)."""
    dt = ac.DTYPES[name]
    issue_rows = np.concatenate([ac.seeded_maxes(dt), ac.edge_maxes(dt)])
    fused, ulp = ac.sensitivity(ac.QuantDomain(dt, issue_rows))
    print(f"{name}: single rounding would move {fused} symbols, a one-ulp factor error {ulp}")
    assert fused >= 50 and ulp >= 300
    dom = ac.QuantDomain(dt, np.concatenate([issue_rows, ac.outside_maxes(dt)]))
    n = len(dom.x)
    x_d, row_d = up(dom.x), up(dom.row)
    fast, special, cvt = out(n), out(n), out(4 * n)
    checked = 0
    for MAX in ac.MAXES:
        f = dom.factors(MAX)
        ah.call("ah_quant_single", x_d, row_d, up(f), float(MAX), fast, special, n=n)
        ah.call("ah_quant_pair", x_d, row_d, up(f), float(MAX), cvt, n=n)
        reg = np.isfinite(f)[dom.row]  # (the largest bf16 denormal is a regular row only while its factor is finite)
        ref = ac.quant_ref(dom.x, f[dom.row], MAX)[reg]
        assert ref.min() >= 0 and ref.max() <= 2 * MAX
        want = ref.astype(np.uint32)
        assert np.array_equal(down(fast)[reg], want), f"quant_fast, MAX {MAX}"
        assert np.array_equal(down(special)[reg] & 0xff, want), f"quant_special, MAX {MAX}"
        got = down(cvt).reshape(4, n)
        for p in range(4):
            keep = np.uint32(0xa5a5a5a5 & ~(0xff << (8 * p)))
            assert np.array_equal(got[p][reg], keep | (want << np.uint32(8 * p))), f"quant_z2 + v_cvt_pk_u8_f32 at byte {p}, MAX {MAX}"
        checked += int(reg.sum())
    print(f"{name}: {checked} elements")


@pytest.mark.parametrize("name", list(ac.DTYPES))
def test_quantise_special_rows_every_x_pattern(harness, name):
    """Rows whose max is zero, inf or NaN, and bf16 denormal maxes whose factor overflows (131 / 75 (max, MAX) pairs),
    with every 16-bit x pattern -- NaN and inf elements too -- through quant_special: 8.6 M / 4.9 M elements."""
    dt = ac.DTYPES[name]
    rows = ac.special_rows(dt)
    allx = ac.widen(np.arange(1 << 16, dtype=np.uint16), dt)
    m = np.array([r[0] for r in rows], np.uint16)
    MAX = np.array([r[1] for r in rows], np.float32)
    f = ac.row_factor(m, MAX, dt)
    x = np.tile(allx, len(rows))
    row = np.repeat(np.arange(len(rows), dtype=np.uint32), 1 << 16)
    got = out(len(x))
    ah.call("ah_quant_special", up(x), up(row), up(f), up(MAX), got, n=len(x))
    want = ac.quant_special_ref(x, f[row], MAX[row])
    assert np.array_equal(down(got), want)


def test_quantise_step_on_the_golden_edge_rows(harness, golden_dir):
    """tests/golden/quant_edge.npz (rows the reference implementation quantised: zero, denormal, inf, NaN maxes among
    them) element by element through the helpers, each row by the rule the kernels pick it with."""
    z = np.load(os.path.join(golden_dir, "quant_edge.npz"))
    xb, sym, scale, bins = z["x"], z["sym"], z["scale"], z["bins"]
    for p in range(xb.shape[0]):
        MAX = int(bins[p]) // 2 - 1
        T, C = xb.shape[1:]
        x = ac.widen(xb[p].ravel(), ac.BF16)
        row = np.repeat(np.arange(T, dtype=np.uint32), C)
        f = ac.row_factor(scale[p], MAX, ac.BF16)
        is_special = ~np.isfinite(f) | ~np.isfinite(ac.widen(scale[p], ac.BF16))
        n = len(x)
        fast, special, cvt = out(n), out(n), out(4 * n)
        ah.call("ah_quant_single", up(x), up(row), up(f), float(MAX), fast, special, n=n)
        ah.call("ah_quant_pair", up(x), up(row), up(f), float(MAX), cvt, n=n)
        want = sym[p].ravel().view(np.uint8).astype(np.uint32)
        sp = is_special[row]
        assert sp.any() and (~sp).any()
        assert np.array_equal(down(special)[sp] & 0xff, want[sp])
        assert np.array_equal(down(fast)[~sp] & 0xff, want[~sp])
        assert np.array_equal(down(cvt)[:n][~sp], np.uint32(0xa5a5a500) | want[~sp])


# ------------------------------------------------------------------ (d) the coder's division
def test_divmod_est_and_rans_put(harness):
    """Every f in 1 .. 65535; x at the quotient steps of 46 chosen and 64 seeded quotients, at the ends of [0, f 2^16) and
    at 64 seeded places: 25.8 M cases.  divmod_est must give x / f and x % f, rans_put the coder's state update."""
    x, f, st = ac.rans_cases()
    n = len(x)
    q, r, put = out(n), out(n), out(n)
    ah.call("ah_rans", up(x), up(f), up(st), q, r, put, n=n)
    wq, wr, wput = ac.rans_ref(x, f, st)
    print(f"{n} cases")
    assert np.array_equal(down(q), wq) and np.array_equal(down(r), wr)
    assert np.array_equal(down(put), wput)


# ------------------------------------------------------------------ (e) the CDF arithmetic
def test_rne_div_every_total(harness):
    """rne_div_u32(n 65504, T, floor(2^32 / T)) for every T in 1 .. 65535 at the places a rounding goes wrong (around
    T / 2, the ends) and 64 seeded n, every n for T <= 1024: 5.2 M cases with 990 exact ties, against integer RNE."""
    n, T = ac.rne_cases()
    v = n * ac.CDF_SCALE
    want, tie = ac.rne_ref(v, T)
    n0, T0 = ac.rne_cases(exhaustive_below=0)
    assert np.count_nonzero(ac.rne_ref(n0 * ac.CDF_SCALE, T0)[1]) >= 200  # (the per-T part alone; the host file holds it too)
    got = out(len(n))
    ah.call("ah_rne_div", up(u32(v)), up(u32(T)), up(u32(ac.rne_magic(T))), got, n=len(n))
    print(f"{len(n)} cases, {int(tie.sum())} ties")
    assert np.array_equal(down(got), u32(want))


def _columns(entry, counts, T, nsym, words, dtype):
    res = out(len(counts) * words, torch.int16 if dtype == np.uint16 else torch.int32, 0x5a5a if dtype == np.uint16 else 0x5a5a5a5a)
    ah.call(entry, up(ac.pack_hreg(counts)), up(u32(T)), up(u32(nsym)), res, n=len(counts))
    return down(res, dtype)


def test_cdf_columns(harness, golden_dir):
    """cdf_column_to_lds / _wide over T in {1, 2, 3, 255, 256, 257, 300, 768, 1000, 4096, 32768, 65535} x nsym in
    {2, 3, 15, 16, 17, 30, 31} (wide: up to 16), 64 histograms each -- all in the first symbol, all in the last, a column
    of ones, seeded flat and peaked ones: every table entry is RNE(N_i 65504 / T) + i, entry 32 stored as 0.  Then the
    histograms of tests/golden/cdf.npz, against the tables the reference implementation wrote."""
    counts, T, nsym = ac.cdf_cases()
    want = ac.cdf_ref(counts, T, nsym)
    assert (want[:, :, 32] == 65536).all()
    got = _columns("ah_cdf_column", counts, T, nsym, 33 * 64, np.uint16).reshape(len(counts), 33, 64)
    assert np.array_equal(got.transpose(0, 2, 1), (want & 0xffff).astype(np.uint16))
    counts, T, nsym = ac.cdf_cases(wide=True)
    got = _columns("ah_cdf_column_wide", counts, T, nsym, 1024, np.uint32).reshape(len(counts), 4, 64, 4)
    assert np.array_equal(got, ac.cdf_wide_ref(ac.cdf_ref(counts, T, nsym)))
    z = np.load(os.path.join(golden_dir, "cdf.npz"))
    for Tg in (1, 7, 16, 128, 236, 250, 256, 768):
        counts, ns, want, real = ac.golden_cdf_cases(z, Tg)
        k = len(counts)
        got = _columns("ah_cdf_column", counts, np.full(k, Tg), ns, 33 * 64, np.uint16).reshape(k, 33, 64)
        assert np.array_equal(got.transpose(0, 2, 1)[real], want[real].astype(np.uint16)), Tg
        narrow = ns <= 16  # (the fixture's second plane: the packed form as well)
        assert narrow.any()
        got = _columns("ah_cdf_column_wide", counts[narrow], np.full(k, Tg)[narrow], ns[narrow], 1024, np.uint32).reshape(-1, 4, 64, 4)
        unwrapped = np.where(np.arange(33) == 32, 65536, want[narrow])
        assert np.array_equal(got.transpose(0, 2, 1, 3)[real[narrow]], ac.cdf_wide_ref(unwrapped).transpose(0, 2, 1, 3)[real[narrow]]), Tg


# ------------------------------------------------------------------ (f) small exact pieces
def test_divmod_small_and_split_divmod_on_the_device(harness):
    """divmod_small for R 2 .. 30, e < 2^15 and split_divmod for R 4 .. 2048, e < 2048 (their stated domains, 0.95 M and
    4.2 M cases), with the reciprocal the kernels compute: fl(1 / R)."""
    for entry, (e, R) in (("ah_divmod_small", ac.divmod_small_cases()), ("ah_split_divmod", ac.split_divmod_cases())):
        rcp = (np.float32(1.0) / R.astype(np.float32)).astype(np.float32)
        q, r = out(len(e)), out(len(e))
        ah.call(entry, up(e), up(R), up(rcp), q, r, n=len(e))
        assert np.array_equal(down(q), e // R) and np.array_equal(down(r), e % R), entry


def test_counts_scale_magic_and_multiply_high(harness):
    """lmc_counts_scale_magic_dev(T) is lmc_format.h's ceil(2^32 / T) for T 2 .. 65535, and the multiply-high of x << 8
    with it is floor(256 x / T) for T 2 .. 256, x <= T."""
    T = np.arange(2, 65536, dtype=np.int64)
    x = np.minimum(T, 255)  # (x << 8 stays in 32 bits whatever T; the values are checked for T <= 256 below)
    scaled, magic = out(len(T)), out(len(T))
    ah.call("ah_counts_scale", up(u32(x)), up(u32(T)), scaled, magic, n=len(T))
    assert np.array_equal(down(magic), u32(((1 << 32) + T - 1) // T))
    T = np.repeat(np.arange(2, 257, dtype=np.int64), 257)
    x = np.tile(np.arange(257, dtype=np.int64), 255)
    T, x = T[x <= T], x[x <= T]
    scaled, magic = out(len(T)), out(len(T))
    ah.call("ah_counts_scale", up(u32(x)), up(u32(T)), scaled, magic, n=len(T))
    assert np.array_equal(down(scaled), u32(256 * x // T))


def test_casts_against_torch(harness):
    """f2bf16 on (h << 16) + {0, 1, 0x7fff, 0x8000, 0x8001, 0xffff} for every 16-bit h (393 216 fp32 patterns: ties, NaN
    payloads, infinities, zeros, denormals, the largest finite bf16) and f2fp16 on every fp16 value, the fp32 midpoints
    between neighbours and one ulp either side, the turn to inf around 65520, fp32 denormals and NaNs (254 242
    patterns), against torch's CPU casts; NaN compared as NaN (and f2bf16's NaN held at 0x7fc0).  And the widening the quantisers read with, every
    pattern of both dtypes."""
    fb = ac.f2bf16_inputs()
    got = out(len(fb))
    ah.call("ah_f2bf16", up(fb), got, n=len(fb))
    g, w = down(got), ac.f2bf16_ref(fb)
    nan_in = (fb & 0x7fffffff) > 0x7f800000
    assert np.array_equal(g[~nan_in], w[~nan_in])
    # NaN: torch's cast has no single answer -- c10::BFloat16's scalar conversion gives 0x7fc0 whatever the payload and
    # sign (torch.tensor(nan).to(bfloat16), and the GPU's cast), the vectorised CPU kernel writes 0xffff.  The helper
    # states the scalar rule: exactly 0x7fc0, and torch's result is a NaN too
    assert nan_in.sum() == 2 * (128 * 6 - 1) and ((w[nan_in] & 0x7fff) > 0x7f80).all() and (g[nan_in] == 0x7fc0).all()
    fb = ac.f2fp16_inputs()
    got = out(len(fb))
    ah.call("ah_f2fp16", up(fb), got, n=len(fb))
    g, w = down(got), ac.f2fp16_ref(fb)
    nan_g, nan_w = (g & 0x7fff) > 0x7c00, (w & 0x7fff) > 0x7c00
    assert g.max() <= 0xffff and np.array_equal(nan_g, nan_w) and np.array_equal(g[~nan_w], w[~nan_w])
    allb = np.arange(1 << 16, dtype=np.uint32)
    for dt in ac.DTYPES.values():
        got = out(len(allb))
        ah.call("ah_h2f", up(allb), dt, got, n=len(allb))
        assert ac.same_floats(down(got), ac.f32_bits(ac.widen(allb.astype(np.uint16), dt))).all()
        if dt == ac.BF16:
            assert np.array_equal(down(got), allb << 16)


def test_transpose64(harness):
    """Every single-bit matrix (4096), the identity, all ones and 256 seeded matrices against numpy; twice is the
    identity."""
    rows = ac.transpose_cases()
    k = len(rows)
    once, twice = out(k * 64, torch.int64, 0x5a5a5a5a5a5a5a5a), out(k * 64, torch.int64, 0x5a5a5a5a5a5a5a5a)
    ah.call("ah_transpose64", up(rows), once, n=k)
    ah.call("ah_transpose64", once, twice, n=k)
    assert np.array_equal(down(once, np.uint64).reshape(k, 64), ac.transpose_ref(rows))
    assert np.array_equal(down(twice, np.uint64).reshape(k, 64), rows)


# ------------------------------------------------------------------ the kernels use what was tested
@pytest.fixture(scope="module")
def ctx():
    native.lib()
    c = native.get_context(0)
    yield c
    c.set_encode_path("auto")


def _encode(ctx, call, layout, ntok, cs, bins):
    stride = native.r16(native.blob_bound(layout.L, cs, layout.H, layout.D))
    n = ntok // cs
    arena = torch.full((n * stride,), 0xa5, dtype=torch.uint8, device=DEV)
    sizes = torch.zeros(n, dtype=torch.int32, device=DEV)
    call(layout, 0, ntok, cs, bins, arena.data_ptr(), stride, sizes.data_ptr())
    torch.cuda.synchronize()
    ctx.raise_on_status("encode")
    sz, host = sizes.cpu().tolist(), arena.cpu().numpy()
    return [host[i * stride:i * stride + sz[i]].tobytes() for i in range(n)]


@pytest.mark.parametrize("name", list(ac.DTYPES))
def test_encoders_on_rows_at_the_decision_points(ctx, oracle, name):
    """L 8, H 2, D 64 (16 planes of 128 channels), bins 4, 6, .. 32 and 23 (every MAX), three 256-token chunks.  Row maxes:
    the short division's edge patterns, their neighbours outside the range, zero, the smallest denormal, the largest
    finite value, inf and NaN, each at every token position mod 8 (the fused kernel picks the division per row PAIR: in-
    and out-of-range rows meet), the rest cycling through the 64 seeded maxes.  A regular row holds its max and the 127
    values whose fl(x * factor) + MAX is nearest a half-integer: about 3000 (bf16 3049, fp16 2886) of the elements move
    with a one-ulp factor error.  The fused kernel, the two kernels and the fixed-width encoder must write the oracle's
    (the fixed-width model's) bytes."""
    dt = ac.DTYPES[name]
    bits, maxes = ac.e2e_chunk(dt)
    moved = ac.e2e_ulp_sensitivity(bits, maxes, dt)
    print(f"{name}: a one-ulp factor error would move {moved} symbols")
    assert moved >= 300
    L, H, D, cs = ac.E2E_L, ac.E2E_H, ac.E2E_D, ac.E2E_CHUNK
    ntok = bits.shape[2]
    code = oracle.BF16 if dt == ac.BF16 else oracle.FP16
    kv = oracle.bits_to_torch(bits, code).reshape(L, 2, ntok, H, D)
    assert np.array_equal(oracle.torch_to_bits(kv.reshape(L, 2, ntok, H * D))[0], bits)
    layout = native.KVLayout.from_chunk(kv.to(DEV), "vllm")
    bins = np.array(ac.E2E_BINS, np.int32)
    coded = [oracle.encode_blob(np.ascontiguousarray(bits[:, :, t:t + cs]), code, H, D, bins) for t in range(0, ntok, cs)]
    fixed = [fm.encode_blob(oracle, np.ascontiguousarray(bits[:, :, t:t + cs]), code, H, D, bins) for t in range(0, ntok, cs)]
    for path in ("fused", "two_kernels"):
        ctx.set_encode_path(path)
        try:
            got = _encode(ctx, ctx.encode_chunks, layout, ntok, cs, ac.E2E_BINS)
        finally:
            ctx.set_encode_path("auto")
        assert [len(b) for b in got] == [len(b) for b in coded], path
        for i in range(len(coded)):
            assert got[i] == coded[i], f"{path}: chunk {i} differs from the oracle's blob"
    got = _encode(ctx, ctx.encode_chunks_fixed, layout, ntok, cs, ac.E2E_BINS)
    for i in range(len(fixed)):
        assert got[i] == fixed[i], f"fixed-width: chunk {i} differs from the model's blob"
