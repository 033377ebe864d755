"""numpy restatement of LMC_MODEL_FIXED (include/lmc_format.h): the reference of the fixed-width blobs' bytes.

TEST INFRASTRUCTURE ONLY.  Quantisation, dequantisation and the static sections (header, bins, scales, scsum) come from
the CPU oracle, which is the same for every model; packing, the check word, the stream directory and the totals are
restated here from the format's text."""
import numpy as np

MODEL_FIXED = 2
NARROW_BINS = 17
TAIL = 16
# header words (lmc_blob_header)
W_T, W_C, W_P, W_G, W_OFF_BINS, W_OFF_SCALES, W_OFF_GDIR, W_OFF_STREAMS, W_STREAM_BYTES, W_TOTAL, W_OFF_SCSUM, W_MODEL = \
    4, 7, 8, 9, 11, 12, 14, 15, 16, 17, 21, 22


def r16(x):
    return (x + 15) & ~15


def stream_bytes(bins, T):
    O = (T + 7) // 8
    return (256 if bins <= NARROW_BINS else 320) * O + TAIL


def static_bytes(L, T, H, D):
    P, G = 2 * L, (H * D + 63) // 64
    return 128 + r16(P) + r16(2 * P * T) + r16(4 * P) + r16(8 * P * G)


def blob_bytes(L, T, H, D, bins):
    G = (H * D + 63) // 64
    return static_bytes(L, T, H, D) + G * sum(stream_bytes(int(b), T) for b in bins)


def check_word(dwords):
    """sum of (2 i + 1) * w_i mod 2^32 over the dwords of lo, then hi, in address order."""
    w = np.asarray(dwords, dtype=np.uint64)
    i = np.arange(len(w), dtype=np.uint64)
    return int(((2 * i + 1) * w).sum() & 0xffffffff)


def pack_stream(s, wide):
    """s: symbols uint8 [T, 64] of one group (lanes past C are 0) -> the stream's bytes."""
    T = s.shape[0]
    O = (T + 7) // 8
    pad = np.zeros((8 * O, 64), np.uint32)
    pad[:T] = s
    o = pad.reshape(O, 8, 64)
    lo = np.zeros((O, 64), np.uint32)
    for k in range(4):
        lo |= ((o[:, k] & 15) | ((o[:, 4 + k] & 15) << 4)) << (8 * k)
    parts = [lo.astype("<u4").tobytes()]
    if wide:
        hi = np.zeros((O, 64), np.uint8)
        for j in range(8):
            hi |= (((o[:, j] >> 4) & 1) << j).astype(np.uint8)
        parts.append(hi.tobytes())
    payload = b"".join(parts)
    chk = check_word(np.frombuffer(payload, "<u4"))
    return payload + np.array([chk, 0, 0, 0], "<u4").tobytes()


def pack_streams(sym, bins):
    """sym int8 [P, T, C] -> (streams section, gdir uint32 [P * G, 2])."""
    P, T, C = sym.shape
    G = (C + 63) // 64
    full = np.zeros((P, T, 64 * G), np.uint8)
    full[:, :, :C] = sym.view(np.uint8)
    out, gdir, at = [], [], 0
    for p in range(P):
        for g in range(G):
            s = pack_stream(full[p, :, 64 * g:64 * g + 64], bins[p] > NARROW_BINS)
            assert len(s) == stream_bytes(int(bins[p]), T)
            gdir.append((at, at + len(s)))
            at += len(s)
            out.append(s)
    return b"".join(out), np.array(gdir, "<u4")


def encode_blob(oracle, kv_bits, dtype, H, D, bins):
    """kv_bits uint16 [L, 2, T, C] -> the LMC_MODEL_FIXED blob."""
    bins = np.asarray(bins, np.int32)
    coded = oracle.encode_blob(kv_bits, dtype, H, D, bins)  # header, bins, scales, scsum: the same for every model
    sym, _ = oracle.quantize(kv_bits, dtype, bins)
    return from_static(coded, sym, bins)


def from_static(coded, sym, bins):
    """The fixed-width blob with the static sections of `coded` (any model's blob of the same chunk) and symbols `sym`."""
    head = np.frombuffer(coded[:128], "<u4").copy()
    streams, gdir = pack_streams(sym, bins)
    off_gdir, off_streams = int(head[W_OFF_GDIR]), int(head[W_OFF_STREAMS])
    head[W_MODEL] = MODEL_FIXED
    head[W_STREAM_BYTES] = len(streams)
    head[W_TOTAL] = off_streams + len(streams)
    gd = gdir.tobytes()
    return head.tobytes() + coded[128:off_gdir] + gd + bytes(off_streams - off_gdir - len(gd)) + streams


def header(blob):
    return np.frombuffer(blob[:128], "<u4")


def stream_spans(blob):
    """[(payload begin, payload end = position of the check word)] of every stream, absolute offsets, (p, g) order."""
    h = header(blob)
    n = int(h[W_P] * h[W_G])
    gdir = np.frombuffer(blob, "<u4", 2 * n, int(h[W_OFF_GDIR])).reshape(n, 2).astype(np.int64)
    base = int(h[W_OFF_STREAMS])
    return [(base + int(b), base + int(e) - TAIL) for b, e in gdir]


def unpack_symbols(blob):
    """-> int8 [P, T, C], checking every stream's check word and tail on the way."""
    h = header(blob)
    T, C, P, G = int(h[W_T]), int(h[W_C]), int(h[W_P]), int(h[W_G])
    O = (T + 7) // 8
    bins = np.frombuffer(blob, np.uint8, P, int(h[W_OFF_BINS]))
    sym = np.zeros((P, 8 * O, 64 * G), np.uint8)
    for i, (b, e) in enumerate(stream_spans(blob)):
        p, g = divmod(i, G)
        payload = np.frombuffer(blob, "<u4", (e - b) // 4, b)
        tail = np.frombuffer(blob, "<u4", 4, e)
        assert tail[0] == check_word(payload) and not tail[1:].any(), f"stream {i}"
        lo = payload[:64 * O].reshape(O, 64)
        s = np.zeros((O, 8, 64), np.uint8)
        for k in range(4):
            byte = (lo >> (8 * k)) & 0xff
            s[:, k] = byte & 15
            s[:, 4 + k] = byte >> 4
        if bins[p] > NARROW_BINS:
            hi = np.frombuffer(blob, np.uint8, 64 * O, b + 256 * O).reshape(O, 64)
            for j in range(8):
                s[:, j] |= ((hi >> j) & 1) << 4
        sym[p, :, 64 * g:64 * g + 64] = s.reshape(8 * O, 64)
    return sym[:, :T, :C].view(np.int8).copy()


def decode_blob(oracle, blob, out_dtype):
    """-> uint16 [L, 2, T, C] in out_dtype."""
    h = header(blob)
    T, P = int(h[W_T]), int(h[W_P])
    bins = np.frombuffer(blob, np.uint8, P, int(h[W_OFF_BINS])).astype(np.int32)
    scales = np.frombuffer(blob, "<u2", P * T, int(h[W_OFF_SCALES])).reshape(P, T)
    return oracle.dequantize(unpack_symbols(blob), scales, int(h[2]), bins, out_dtype)
