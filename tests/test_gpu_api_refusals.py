"""The C API's refusals as a table: one row per (entry point, refusal class).

The entry points are the ones whose argument checks and staging are shared code in lmc_api.hip: the blob-arena checks of
the encodes (encode_dst_ok), the chunk geometry of the transcodes and of lmc_pack_blobs, and the store / load staging of
the legs.  No row launches anything: a refused call returns its code, and after a device synchronize the job's status
word and every buffer the call could have written -- all prefilled with a byte pattern -- are what they were.  Then one
valid call of the same entry point succeeds on the same context.

Every pointer of a refused call is a live allocation with room for the geometry the call names, except the one null or
misaligned argument a row is about (refused on the host before anything else is looked at): a refusal that went missing
would write into memory this test owns and fail an assertion.  Two rows name a job too large to give room to; they pass
the smallest shape's buffers and say so where they are built.

The smallest shape serves: L = 1, H = 1, D = 8, bf16, chunks of 4 tokens, 2 chunks; an LMC_PAGED_SPLIT ("NHDB") cache of
blocks of 4 where an entry point takes one; H = 129 for planes of more than 1024 channels."""
import ctypes

import pytest
import torch

from lmcache_amd import native

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
L, H, D, CS, N = 1, 1, 8, 4, 8
NCH = N // CS
H_WIDE = 129              # C = 1032: past what the NHDB encode instances take
BINS = [16, 32]
PATTERN, WORD = 0xC3, 0x5A5A5A5A
BF16 = native.BF16
INVALID, NOT_LAYERWISE = native.ERR_INVALID, native.NOT_LAYERWISE
MAX_BINS = native.MAX_BINS
BIG = 32769               # chunks of 65535 tokens that hold 2^31 tokens: 32768 * 65535 < 2^31 <= 32769 * 65535
assert (BIG - 1) * 65535 < 0x80000000 <= BIG * 65535


def stream():
    return native.current_stream_ptr(torch.device(DEV))


def filled(nbytes):
    return torch.full((int(nbytes),), PATTERN, dtype=torch.uint8, device=DEV)


def pinned(nbytes):
    p = native.PinnedBuffer(int(nbytes))
    p.tensor.fill_(PATTERN)
    return p


def layout(kind, fill=False):
    """-> (KVLayout, (L, H, D), the tensor behind it).  kind: "rows", "fp8" (rows), "c12" (rows of 12 channels), "nhdb",
    "nhdb_wide".  fill: a destination -- the byte pattern instead of data."""
    h, d = (H_WIDE if kind == "nhdb_wide" else H), (12 if kind == "c12" else D)
    dt = torch.float8_e4m3fn if kind == "fp8" else torch.bfloat16
    shape = (2, N // 4, h, d, 4) if kind.startswith("nhdb") else (L, 2, N, h, d)
    if fill:
        n = 1
        for s in shape:
            n *= s
        t = filled(n * native.elem_bytes(native.dtype_code(dt))).view(dt).view(shape)
    else:
        t = torch.randn(shape, generator=torch.Generator().manual_seed(7)).to(dt).to(DEV)
    if kind.startswith("nhdb"):
        lay = native.KVLayout.paged([t], torch.arange(N, dtype=torch.int64, device=DEV), 4, "NHDB")
    else:
        lay = native.KVLayout.from_chunk(t, "vllm")
    return lay, (L, h, d), t


class Case:
    """One entry point's call: `a` holds its arguments by name (a row spoils a copy), `outputs` everything it may write."""

    def __init__(self, a, outputs, call, keep=()):
        self.a, self.outputs, self.call, self.keep = a, outputs, call, keep


class Env:
    """The context, the job's status word and the inputs every row shares (made once, never written again)."""

    def __init__(self):
        self.lib = native.lib()
        self.ctx = native.get_context(0)
        self.word = native.PinnedBuffer(64)
        self.words = self.word.tensor.view(torch.int32)
        src, _, self.kv = layout("rows")
        self.stride = native.r16(native.blob_bound(L, CS, H, D))
        self.coded, self.coded_sizes = self._encode(self.ctx.encode_chunks, src)
        self.fixed, self.fixed_sizes = self._encode(self.ctx.encode_chunks_fixed, src)
        # the same blobs in pinned host memory, and as a pack there
        self.host = pinned(NCH * self.stride)
        self.host_off, self.host_sizes = pinned(8 * (NCH + 1)), pinned(4 * NCH)
        self.ctx.store_chunks(src, 0, N, CS, BINS, self.host.ptr, NCH * self.stride, self.host_off.ptr, self.host_sizes.ptr)
        self.pack_cap = native.pack_bound(NCH, L, CS, H, D)
        self.pack, pack_sizes = pinned(self.pack_cap), pinned(4 * NCH)
        self.ctx.store_pack(src, 0, N, CS, BINS, self.pack.ptr, self.pack_cap, pack_sizes.ptr)
        torch.cuda.synchronize()
        assert self.ctx.status(clear=True) == 0
        self.pack_bytes = int(native.pack_info(self.pack.ptr, self.pack_cap).total_bytes)

    def _encode(self, call, src):
        region = filled(NCH * self.stride)
        sizes = torch.zeros(NCH, dtype=torch.int32, device=DEV)
        call(src, 0, N, CS, BINS, region.data_ptr(), self.stride, sizes.data_ptr())
        torch.cuda.synchronize()
        assert self.ctx.status(clear=True) == 0
        return region, sizes

    def set_word(self, v):
        self.words[0] = v

    def get_word(self):
        return int(self.words[0]) & 0xffffffff


@pytest.fixture(scope="module")
def env():
    return Env()


# ---- the entry points ---------------------------------------------------------------------------------------------------
def encode_case(env, name, kind):
    """lmc_encode_chunks*, lmc_encode_layers_begin*: (src, range, bins, blobs, blob_stride, sizes)."""
    src, (l, h, d), t = layout(kind)
    stride = native.r16(native.blob_bound(l, CS, h, d))
    blobs, sizes = filled(NCH * stride + 16), filled(64)  # (+16: the misaligned row's blobs + 8 has its room)
    a = dict(src=src, tok_begin=0, tok_end=N, cs=CS, bins=BINS, blobs=blobs.data_ptr(), stride=stride, sizes=sizes.data_ptr(),
             bound=native.blob_bound(l, CS, h, d))
    fn = getattr(env.lib, name)

    def call(a):
        args = (env.ctx.handle, ctypes.byref(a["src"].struct), a["tok_begin"], a["tok_end"], a["cs"], native.Context._bins(a["bins"]),
                a["blobs"], a["stride"], a["sizes"], env.word.ptr)
        if "layers" not in name:
            return fn(*args, stream())
        job = ctypes.c_void_p()
        rc = fn(*args, ctypes.byref(job))
        assert (rc == 0) == bool(job.value)
        if job.value:  # accepted: the job is aborted before a layer is launched
            assert env.lib.lmc_encode_layers_abort(env.ctx.handle, job) == 0
        return rc
    return Case(a, [blobs, sizes], call, keep=(t,))


def store_case(env, name, kind):
    """lmc_store_chunks, lmc_store_pack, lmc_store_pack_parts: the encode's source and range, `blobs` the host arena / the
    pack (lmc_store_pack_parts: a device region)."""
    src, (l, h, d), t = layout(kind)
    cap = NCH * native.r16(native.blob_bound(l, CS, h, d)) if name == "lmc_store_chunks" else native.pack_bound(NCH, l, CS, h, d)
    dst = filled(cap + 16) if name == "lmc_store_pack_parts" else pinned(cap + 16)
    dst_ptr = dst.data_ptr() if name == "lmc_store_pack_parts" else dst.ptr
    offs, sizes, info = pinned(8 * 8), pinned(64), pinned(8 * 4)
    a = dict(src=src, tok_begin=0, tok_end=N, cs=CS, bins=BINS, blobs=dst_ptr, cap=cap)
    fn = getattr(env.lib, name)

    def call(a):
        head = (env.ctx.handle, ctypes.byref(a["src"].struct), a["tok_begin"], a["tok_end"], a["cs"], native.Context._bins(a["bins"]),
                a["blobs"], a["cap"])
        if name == "lmc_store_chunks":
            return fn(*head, offs.ptr, sizes.ptr, env.word.ptr, stream())
        if name == "lmc_store_pack":
            return fn(*head, sizes.ptr, env.word.ptr, stream())
        return fn(*head, sizes.ptr, 2, info.ptr, None, env.word.ptr, stream())
    outs = [dst if name == "lmc_store_pack_parts" else dst.tensor, offs.tensor, sizes.tensor]
    # (lmc_store_pack_parts clears the parts' info words on the host once the job is accepted: they are no output of a refusal
    # either, so they are watched too)
    return Case(a, outs + [info.tensor], call, keep=(t, dst, offs, sizes, info))


def table(ptrs, n=None):
    """Device int64 table of `ptrs`, repeated up to n entries."""
    ptrs = list(ptrs)
    return torch.tensor((ptrs * ((n or len(ptrs)) // len(ptrs) + 1))[:n or len(ptrs)], dtype=torch.int64, device=DEV)


def blob_case(env, name, kind="rows"):
    """lmc_transcode_fixed, lmc_transcode_to_fixed, lmc_pack_blobs: blobs of earlier stores through a pointer table, their
    geometry as numbers.  The tables have `tables` entries (the two blobs over and over past the second)."""
    fixed_in = name == "lmc_transcode_fixed"
    region, rsizes = (env.fixed, env.fixed_sizes) if fixed_in else (env.coded, env.coded_sizes)
    stride = 2 * env.stride  # (room for the rows that name 12 channels)
    out, sizes = filled(NCH * stride + 16), filled(4 * 65536)
    cap = native.pack_bound(NCH, L, CS, H, 2 * D)
    a = dict(nchunks=NCH, L=L, H=H, D=D, dtype=BF16, cs=CS, ntokens=N, bins=BINS, blobs=out.data_ptr(), stride=stride,
             sizes=sizes.data_ptr(), cap=cap, tables=NCH, out_ptrs=True, bound=native.blob_bound(L, CS, H, D))
    if name == "lmc_pack_blobs":
        out = filled(cap + 16)
        a["blobs"] = out.data_ptr()
    fn = getattr(env.lib, name)
    keep = []

    def call(a):
        n = a["tables"]
        ptrs = table([region.data_ptr() + i * env.stride for i in range(NCH)], n)
        room = torch.tensor((rsizes.cpu().tolist() * (n // NCH + 1))[:n], dtype=torch.int32, device=DEV)
        keep[:] = [ptrs, room]
        head = (env.ctx.handle, ptrs.data_ptr(), room.data_ptr(), a["nchunks"], a["L"], a["H"], a["D"])
        if name == "lmc_pack_blobs":
            return fn(*head, a["cs"], a["ntokens"], a["blobs"], a["cap"], env.word.ptr, stream())
        head += (a["dtype"], a["cs"], a["ntokens"], native.Context._bins(a["bins"]))
        if fixed_in:
            return fn(*head, a["blobs"], a["stride"], a["sizes"], env.word.ptr, stream())
        outs = table([out.data_ptr() + i * stride for i in range(NCH)], n)
        obytes = torch.full((n,), stride, dtype=torch.int32, device=DEV)
        keep.extend([outs, obytes])
        return fn(*head, outs.data_ptr() if a["out_ptrs"] else None, obytes.data_ptr(), env.word.ptr, stream())
    return Case(a, [out, sizes], call, keep=keep)


def load_case(env, name, kind="rows"):
    """lmc_load_pack, lmc_load_pack_post, lmc_unpack_blobs (the pinned pack), lmc_load_chunks (the pinned blobs)."""
    dst, _, t = layout(kind, fill=True)
    blobs = filled(NCH * env.stride)
    a = dict(chunk_begin=0, nchunks=NCH, cs=CS, dst=dst, ptrs=True)
    fn = getattr(env.lib, name)

    def call(a):
        n = max(a["nchunks"], 1)
        if name == "lmc_unpack_blobs":
            ptrs = (ctypes.c_void_p * n)(*[blobs.data_ptr() + (i % NCH) * env.stride for i in range(n)])
            caps = (ctypes.c_uint32 * n)(*[env.stride] * n)
            return fn(env.ctx.handle, env.pack.ptr, env.pack_bytes, a["chunk_begin"], a["nchunks"], ptrs, caps, env.word.ptr, stream())
        if name == "lmc_load_chunks":
            offs = env.host_off.tensor.view(torch.int64).tolist()
            ptrs = (ctypes.c_void_p * NCH)(*[env.host.ptr + offs[i] for i in range(NCH)])
            sizes = (ctypes.c_uint32 * NCH)(*[int(v) & 0xffffffff for v in env.host_sizes.tensor.view(torch.int32).tolist()])
            return fn(env.ctx.handle, ptrs if a["ptrs"] else None, sizes, a["nchunks"], ctypes.byref(a["dst"].struct), 0, a["cs"], 0,
                      None, env.word.ptr, stream())
        args = (env.ctx.handle, env.pack.ptr, env.pack_bytes, a["chunk_begin"], a["nchunks"], ctypes.byref(a["dst"].struct), 0, 0, None,
                env.word.ptr, stream())
        return fn(*args, None) if name == "lmc_load_pack_post" else fn(*args)
    return Case(a, [t.view(torch.uint8), blobs], call)


def decode_case(env, name, kind="rows"):
    """lmc_decode_chunks (the coded blobs), lmc_decode_chunks_fixed_schedule (the fixed-width ones): neither takes an NHDB
    destination."""
    dst, _, t = layout(kind, fill=True)
    a = dict(dst=dst)
    keep = []

    def call(a):
        if name == "lmc_decode_chunks":
            return env.lib.lmc_decode_chunks(env.ctx.handle, env.coded.data_ptr(), env.stride, NCH, ctypes.byref(a["dst"].struct), 0, CS,
                                             env.word.ptr, stream())
        ptrs = table([env.fixed.data_ptr() + i * env.stride for i in range(NCH)])
        keep[:] = [ptrs]
        ends = (ctypes.c_int32 * 1)(L)
        return env.lib.lmc_decode_chunks_fixed_schedule(env.ctx.handle, ptrs.data_ptr(), int(env.fixed_sizes.max()), NCH,
                                                        ctypes.byref(a["dst"].struct), 0, CS, 1, ends, None, None, env.word.ptr, stream())
    return Case(a, [t.view(torch.uint8)], call, keep=keep)


# entry point -> (how its case is built, the source / destination it is given when nothing is wrong with it)
ENCODES = {"lmc_encode_chunks": "rows", "lmc_encode_chunks_split": "nhdb", "lmc_encode_chunks_fixed": "rows",
           "lmc_encode_chunks_fixed_split": "nhdb", "lmc_encode_layers_begin": "nhdb", "lmc_encode_layers_begin_fixed": "nhdb"}
STORES = ["lmc_store_chunks", "lmc_store_pack", "lmc_store_pack_parts"]
ENTRIES = {name: (encode_case, kind) for name, kind in ENCODES.items()}
ENTRIES.update({name: (store_case, "nhdb") for name in STORES})
ENTRIES.update({name: (blob_case, "rows") for name in ("lmc_transcode_fixed", "lmc_transcode_to_fixed", "lmc_pack_blobs")})
ENTRIES.update({name: (load_case, "rows") for name in ("lmc_load_pack", "lmc_load_pack_post", "lmc_unpack_blobs", "lmc_load_chunks")})
ENTRIES.update({name: (decode_case, "rows") for name in ("lmc_decode_chunks", "lmc_decode_chunks_fixed_schedule")})

# ---- the refusal classes: what a row spoils in the arguments, or the kind of source / destination it passes -----------------
SPOIL = {
    "blobs null": lambda a: a.update(blobs=None),
    "blobs misaligned": lambda a: a.update(blobs=a["blobs"] + 8),
    "blob_stride unaligned": lambda a: a.update(stride=a["stride"] + 8),
    "blob_stride below the bound": lambda a: a.update(stride=native.r16(a["bound"]) - 16),
    "bins 3": lambda a: a.update(bins=[16, 3]),
    "bins MAX + 1": lambda a: a.update(bins=[16, MAX_BINS + 1]),
    "tok_end <= tok_begin": lambda a: a.update(tok_begin=CS, tok_end=CS),
    "chunk_tokens 0": lambda a: a.update(cs=0),
    "chunk_tokens 65536": lambda a: a.update(cs=65536),
    "C not a multiple of 8": lambda a: a.update(D=12),
    "ntokens too small": lambda a: a.update(ntokens=(NCH - 1) * CS),
    "ntokens too large": lambda a: a.update(ntokens=NCH * CS + 1),
    # chunks of 65535 tokens: nothing else is wrong with the count.  lmc_transcode_to_fixed gets tables of BIG entries over
    # its two blobs and two output slots (a missing refusal would meet blobs of the wrong length and flag them).  The
    # output arena lmc_transcode_fixed would need for these chunks is 140 GB: it gets the smallest shape's arena and that
    # arena's stride, so that the blob_stride check stands behind this one
    "ntokens > 0x7fffffff": lambda a: a.update(nchunks=BIG, cs=65535, ntokens=0x80000000, tables=BIG, stride=native.r16(a["bound"])),
    "dtype fp8": lambda a: a.update(dtype=native.FP8_E4M3),
    "dtype unknown": lambda a: a.update(dtype=4),
    "out_ptrs null": lambda a: a.update(out_ptrs=False),
    # P * nchunks = 66 * 65535 > 2^22 (L = 32 would be 64 * 65535 = 2^22 - 64: accepted).  Nothing of that size is allocated:
    # the call is refused before it reads a blob, and the pack's capacity stays the smallest shape's
    "P * nchunks > 2^22": lambda a: a.update(L=33, nchunks=65535, ntokens=65535 * CS, tables=65535),
    "chunk_begin outside the pack": lambda a: a.update(chunk_begin=NCH, nchunks=1),
    "chunk_begin negative": lambda a: a.update(chunk_begin=-1, nchunks=1),
    "nchunks outside the pack": lambda a: a.update(chunk_begin=1, nchunks=NCH),
    "nchunks negative": lambda a: a.update(nchunks=-1),
    "nchunks 0": lambda a: a.update(nchunks=0),
    "host pointers null": lambda a: a.update(ptrs=False),
    # lmc_encode_layers_begin: chunks below LMC_COUNTS_T_MIN = 2 tokens are not for the counts-only coder; the fixed-width
    # model has no coder and takes the same arguments
    "chunk_tokens below LMC_COUNTS_T_MIN": lambda a: a.update(cs=1, tok_end=NCH),
}
KIND = {"fp8 source": "fp8", "C not a multiple of 8": "c12", "NHDB where none is taken": "nhdb", "NHDB of C > 1024": "nhdb_wide"}


def rows():
    out = []

    def add(name, cls, rc=INVALID):
        out.append(pytest.param(name, cls, rc, id=f"{name[4:]}-{cls.replace(' ', '_')}"))
    arena = ["blobs null", "blobs misaligned", "blob_stride unaligned", "blob_stride below the bound"]
    bins = ["bins 3", "bins MAX + 1"]
    job = ["tok_end <= tok_begin", "chunk_tokens 0", "chunk_tokens 65536", "C not a multiple of 8"]
    for name in ENCODES:
        for cls in arena + bins + job:
            add(name, cls)
        if "fixed" in name:
            add(name, "fp8 source")
        add(name, "NHDB of C > 1024" if ENCODES[name] == "nhdb" else "NHDB where none is taken")
    add("lmc_encode_layers_begin", "chunk_tokens below LMC_COUNTS_T_MIN", NOT_LAYERWISE)
    add("lmc_encode_layers_begin_fixed", "chunk_tokens below LMC_COUNTS_T_MIN", 0)  # accepted, then aborted
    for name in STORES:
        for cls in arena[:2] + bins + job + ["NHDB of C > 1024"]:
            add(name, cls)
    geometry = ["chunk_tokens 0", "chunk_tokens 65536", "C not a multiple of 8", "ntokens too small", "ntokens too large"]
    for name in ("lmc_transcode_fixed", "lmc_transcode_to_fixed"):
        for cls in geometry + bins + ["ntokens > 0x7fffffff", "dtype fp8", "dtype unknown"]:
            add(name, cls)
    for cls in arena:
        add("lmc_transcode_fixed", cls)
    add("lmc_transcode_to_fixed", "out_ptrs null")
    for cls in geometry + arena[:2] + ["P * nchunks > 2^22"]:
        add("lmc_pack_blobs", cls)
    for name in ("lmc_load_pack", "lmc_load_pack_post", "lmc_unpack_blobs"):
        for cls in ("chunk_begin outside the pack", "chunk_begin negative", "nchunks outside the pack", "nchunks negative"):
            add(name, cls)
    add("lmc_unpack_blobs", "nchunks 0")
    for cls in ("chunk_tokens 0", "nchunks 0", "host pointers null", "C not a multiple of 8"):
        add("lmc_load_chunks", cls)
    add("lmc_decode_chunks", "NHDB where none is taken")
    add("lmc_decode_chunks_fixed_schedule", "NHDB where none is taken")
    return out


def words(t):
    return t.reshape(-1).view(torch.uint8).clone()


@pytest.mark.parametrize("name,cls,want", rows())
def test_a_refused_call_queues_nothing_and_the_next_valid_call_succeeds(env, name, cls, want):
    build, good_kind = ENTRIES[name]
    good = build(env, name, good_kind)
    by_kind = cls in KIND and "D" not in good.a  # (an entry point that takes its geometry as numbers has no layout to spoil)
    bad = build(env, name, KIND[cls]) if by_kind else good
    a = dict(bad.a)
    if not by_kind:
        SPOIL[cls](a)
    before = [words(o) for o in bad.outputs]
    env.set_word(WORD)
    rc = bad.call(a)
    torch.cuda.synchronize()
    assert rc == want, (rc, env.lib.lmc_last_hip_error())
    assert env.get_word() == WORD, "the job's status word"
    assert env.ctx.status() == 0, "the context's status word"
    for o, b in zip(bad.outputs, before):
        assert torch.equal(words(o), b), "a refused call wrote to its output"
    env.set_word(0)
    assert good.call(good.a) == 0
    torch.cuda.synchronize()
    assert env.get_word() == 0 and env.ctx.status(clear=True) == 0
    if "layers" not in name:  # (begin + abort launches nothing)
        assert any(not bool((words(o) == PATTERN).all()) for o in good.outputs), "the valid call wrote nothing"
