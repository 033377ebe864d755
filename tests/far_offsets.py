"""Plain helpers of tests/test_gpu_far_offsets.py (GPU) and tests/test_far_offsets_host.py (CPU): KV layouts whose
offsets from a plane's base pass 2^31 and 2^32 bytes, described in integers, and the checker of the arena they live in.

One allocation -- the ARENA -- holds every such layout.  Its first 2 GiB are a guard, every plane base lies a few KiB
behind them, and the layouts reach 4 GiB + 256 MiB further.  A layout is a Spec: byte offsets only (base, plane, block,
token, head), from which come
  - the byte offset of every head row (RowsSpec) or element (SplitSpec) of the logical KV [L, 2, T, H, D],
  - the torch.as_strided views of the arena that native.KVLayout.paged / from_chunk take,
  - the SAFETY PROPERTY (unsafe_addresses): every address a layout describes lies inside the arena, and so does that
    address with any ONE of its offsets (plane, block, token, head) reduced mod 2^32 or sign-extended from 32 bits.  A kernel
    that narrows one offset then misplaces data inside the arena, where check_arena finds it, instead of faulting.
The GPU tests take their specs from REGISTRY only, and the CPU test checks the property for every entry of it.

The arena is filled with FILL once.  Data are placed and looked at through WINDOW-byte slices of the arena (plain slices:
no index arithmetic of torch's own on a 6 GiB tensor), check_arena compares the windows that hold expected bytes with
their expected image and counts, slab by slab, that nothing outside them has lost the fill pattern."""
import numpy as np
import torch

GIB = 1 << 30
GUARD = 2 * GIB
ARENA_BYTES = GUARD + 4 * GIB + 256 * (1 << 20)
FILL = 0xA5
WINDOW = 4096
SLAB = 256 << 20
BASE = GUARD + 64  # plane (layer 0, K) of every layout; the 64: 2^31 and 2^32 from the guard's end fall inside a token row

L, H, D, T, CS = 2, 2, 64, 104, 40  # two fused chunks of 40 tokens and a ragged one of 24
PLANE_GAP = 4096        # interleaved paged planes: K0, V0, K1, V1 one block apart ...
STRIDE_BLOCK = 16384    # ... in a block slot of 16 KiB
PLANE_FAR = 1503238656  # dense views: ~1.4 GiB between planes, the fourth begins above 2^32 bytes
NUM_BLOCKS = (ARENA_BYTES - BASE) // STRIDE_BLOCK
B31, B32 = (1 << 31) // STRIDE_BLOCK, (1 << 32) // STRIDE_BLOCK
# byte offset from the plane base: the block that ends at 2^31 and the one that starts there, 0, the same two around
# 2^32, the arena's last block; three neighbours for the mappings that need nine blocks (block size 12)
BLOCKS = [B31 - 1, B31, 0, B32 - 1, B32, NUM_BLOCKS - 1, B31 + 1, B32 + 1, B31 - 2]


def mod32(x):
    return np.asarray(x, np.int64) & 0xffffffff


def sext32(x):
    return ((np.asarray(x, np.int64) & 0xffffffff) ^ 0x80000000) - 0x80000000


def slot_table(bs, swapped, ntok=T, blocks=BLOCKS):
    """Block-ordered runs: token t in block blocks[t // bs] at offset t % bs (what the decoder's eight-token path and the
    split copy's fast tiles need).  swapped: two neighbours exchanged inside every block and one pair across two blocks
    -- no group of eight is a run any more, no tile either."""
    pos = np.arange(ntok)
    slots = np.asarray(blocks, np.int64)[pos // bs] * bs + pos % bs
    if swapped:
        for b in range((ntok + bs - 1) // bs):
            i = b * bs + 3
            if i + 1 < ntok:
                slots[[i, i + 1]] = slots[[i + 1, i]]
        slots[[2 * bs + 6, 3 * bs + 1]] = slots[[3 * bs + 1, 2 * bs + 6]]
    assert len(np.unique(slots)) == ntok
    return slots


class Spec:
    """Common part: planes in (layer, kv) order at base + plane_off[2 l + kv]; paged through `slots`."""

    def __init__(self, name, kind, esz, base, plane_off, stride_token, stride_head, slots=None, bs=0, stride_block=0,
                 ntok=T, nl=L, nh=H, hd=D, chunk=CS):
        self.name, self.kind, self.esz, self.base = name, kind, esz, int(base)
        self.plane_off = np.asarray(plane_off, np.int64)
        self.stride_token, self.stride_head, self.stride_block = int(stride_token), int(stride_head), int(stride_block)
        self.slots = None if slots is None else np.asarray(slots, np.int64)
        self.bs, self.ntok, self.L, self.H, self.D, self.chunk = bs, ntok, nl, nh, hd, chunk
        assert len(self.plane_off) == 2 * nl

    def with_(self, name, **kw):
        s = object.__new__(type(self))
        s.__dict__.update(self.__dict__)
        s.__dict__.update(kw)
        s.name = name
        return s

    @property
    def paged(self):
        return self.slots is not None

    def block_off(self):
        return (self.slots // self.bs) * self.stride_block if self.paged else np.zeros(self.ntok, np.int64)

    def head_off(self):
        return np.arange(self.H, dtype=np.int64) * self.stride_head

    def _el(self, nbytes):
        assert nbytes % self.esz == 0
        return int(nbytes) // self.esz

    def _plane_views(self, arena, dt, size, stride):
        """Per layer an as_strided view [2, *size] of the arena: K and V one plane gap apart."""
        a = arena.view(dt)
        out = []
        for l in range(self.L):
            gap = self.plane_off[2 * l + 1] - self.plane_off[2 * l]
            out.append(torch.as_strided(a, (2,) + size, (self._el(gap),) + stride, self._el(self.base + self.plane_off[2 * l])))
        return out


class RowsSpec(Spec):
    """Token rows.  kind "NBHD" / "NHBD": paged blocks; "vllm" / "huggingface": a dense chunk [L,2,T,H,D] / [L,2,H,T,D]."""

    def token_off(self):
        if self.paged:
            return (self.slots % self.bs) * self.stride_token
        return np.arange(self.ntok, dtype=np.int64) * self.stride_token

    def components(self):
        """The offsets an address is the sum of (bytes; the values each can take) and the bytes accessed there."""
        return dict(plane=self.plane_off, block=np.unique(self.block_off()), token=np.unique(self.token_off()),
                    head=self.head_off()), self.D * self.esz

    def row_offsets(self):
        """-> int64 [L, 2, T, H]: arena byte offset of the head row (D elements) of every (layer, kv, token, head)."""
        tok = self.block_off() + self.token_off()
        return (self.base + self.plane_off.reshape(self.L, 2, 1, 1) + tok.reshape(1, 1, -1, 1) + self.head_off().reshape(1, 1, 1, -1))

    def pieces(self, data, tok=None, layers=None):
        """(offsets [n], bytes [n, D * esz]) of data uint8 [l, 2, t, H, D * esz]: the rows of layers `layers` (a slice) at
        the layout's tokens `tok` (a slice or an index array); all of them by default."""
        off = self.row_offsets()
        if layers is not None:
            off = off[layers]
        if tok is not None:
            off = off[:, :, tok]
        assert off.shape == data.shape[:4] and data.shape[4] == self.D * self.esz, (off.shape, data.shape)
        return off.reshape(-1), data.reshape(-1, data.shape[4])

    def views(self, arena, dt):
        e = self._el
        if self.kind in ("NBHD", "NHBD"):
            nb = int(self.slots.max()) // self.bs + 1
            if self.kind == "NBHD":
                return self._plane_views(arena, dt, (nb, self.bs, self.H, self.D),
                                         (e(self.stride_block), e(self.stride_token), e(self.stride_head), 1))
            return self._plane_views(arena, dt, (nb, self.H, self.bs, self.D),
                                     (e(self.stride_block), e(self.stride_head), e(self.stride_token), 1))
        sl, skv = self.plane_off[2] - self.plane_off[0], self.plane_off[1] - self.plane_off[0]
        assert list(self.plane_off) == [l * sl + kv * skv for l in range(self.L) for kv in range(2)]
        if self.kind == "vllm":
            size, stride = (self.L, 2, self.ntok, self.H, self.D), (e(sl), e(skv), e(self.stride_token), e(self.stride_head), 1)
        else:
            size, stride = (self.L, 2, self.H, self.ntok, self.D), (e(sl), e(skv), e(self.stride_head), e(self.stride_token), 1)
        return torch.as_strided(arena.view(dt), size, stride, e(self.base))


class SplitSpec(Spec):
    """kind "NHDB" (include/lmc_hip.h: LMC_PAGED_SPLIT): per block and head one dense run of D * bs elements; K in
    x-element granules (x = 16 / esz), V token-innermost."""

    def components(self):
        inner = np.arange(self.D * self.bs, dtype=np.int64) * self.esz
        return dict(plane=self.plane_off, block=np.unique(self.block_off()), token=inner, head=self.head_off()), self.esz

    def element_offsets(self):
        """-> int64 [L, 2, T, H, D]: the header's K / V address formulas, in bytes."""
        x = 16 // self.esz
        w = (self.slots % self.bs).reshape(-1, 1, 1)
        d = np.arange(self.D, dtype=np.int64).reshape(1, 1, -1)
        k = (d // x) * (self.bs * x) + w * x + d % x
        v = d * self.bs + w
        inner = np.stack([k, v]) * self.esz                                      # [2, T, 1, D]
        outer = self.block_off().reshape(-1, 1, 1) + self.head_off().reshape(1, -1, 1)  # [T, H, 1]
        return self.base + self.plane_off.reshape(self.L, 2, 1, 1, 1) + (outer + inner)[None]

    def pieces(self, data, tok=None, layers=None):
        off = self.element_offsets()
        if layers is not None:
            off = off[layers]
        if tok is not None:
            off = off[:, :, tok]
        assert off.shape[:4] == data.shape[:4] and data.shape[4] == self.D * self.esz
        return off.reshape(-1), data.reshape(-1, self.esz)

    def views(self, arena, dt):
        e = self._el
        nb = int(self.slots.max()) // self.bs + 1
        return self._plane_views(arena, dt, (nb, self.H, self.D, self.bs), (e(self.stride_block), e(self.stride_head), self.bs, 1))


# ------------------------------------------------------------------ the layouts of the GPU tests
INTERLEAVED = [p * PLANE_GAP for p in range(2 * L)]


def paged_rows(kind, esz, bs, swapped):
    name = f"{kind}_e{esz}_bs{bs}_{'swapped' if swapped else 'runs'}"
    st, sh = (H * D * esz, D * esz) if kind == "NBHD" else (D * esz, bs * D * esz)
    assert bs * H * D * esz <= PLANE_GAP
    return RowsSpec(name, kind, esz, BASE, INTERLEAVED, st, sh, slot_table(bs, swapped), bs, STRIDE_BLOCK)


def paged_split(esz, swapped, bs=16):
    assert bs * H * D * esz <= PLANE_GAP
    return SplitSpec(f"NHDB_e{esz}_bs{bs}_{'swapped' if swapped else 'runs'}", "NHDB", esz, BASE, INTERLEAVED, 0, D * bs * esz,
                     slot_table(bs, swapped), bs, STRIDE_BLOCK)


def dense(kind, esz):
    far = [(2 * l + kv) * PLANE_FAR for l in range(L) for kv in range(2)]
    st, sh = (H * D * esz, D * esz) if kind == "vllm" else (D * esz, T * D * esz)
    return RowsSpec(f"dense_{kind}_e{esz}", kind, esz, BASE, far, st, sh)


# The decoder's destination limits (lmc_api.hip: decode_dst_ok; include/lmc_hip.h).  The strides here are bytes.
DESC_RANGE = 0xfffffff0


def row_span(spec):
    """Bytes from the start of a token row to the end of its last channel."""
    return (spec.H - 1) * spec.stride_head + spec.D * spec.esz


def decode_dst_ok(spec, chunk_tokens):
    """The guard's inequalities restated on a spec: the store's scalar offset (`reach`) plus a row must fit the
    descriptor's range."""
    if spec.stride_head < 0 or spec.stride_token < 0:
        return False
    if spec.paged:
        reach = 7 * spec.stride_token if spec.stride_token < (1 << 28) else 0
    else:
        reach = (chunk_tokens - 1) * spec.stride_token
    return reach + row_span(spec) <= DESC_RANGE


def head_stride_limit(esz=2, over=0):
    """A huggingface chunk of H = 2, decoded in chunks of CS tokens, in which the last channel of the second head of a
    chunk's last row ends exactly at the descriptor's range (over = 0), or `over` elements further.  Planes 16 KiB apart:
    a plane's first head is T rows of D elements."""
    st = D * esz
    sh = DESC_RANGE - D * esz - (CS - 1) * st + over * esz
    planes = [p * 16384 for p in range(2 * L)]
    assert T * D * esz <= 16384
    return RowsSpec(f"head_stride_limit_e{esz}_over{over}", "huggingface", esz, BASE, planes, st, sh)


def token_stride_limit(esz=2, over=0):
    """A vllm chunk decoded as ONE chunk of T tokens whose last row ends as far from the first row's start as the
    descriptor's range allows (rows ~40 MiB apart), or `over` elements per row further."""
    st = (DESC_RANGE - H * D * esz) // (T - 1) // esz * esz + over * esz
    return RowsSpec(f"token_stride_limit_e{esz}_over{over}", "vllm", esz, BASE, INTERLEAVED, st, D * esz, chunk=T)


def paged_head_stride_limit(esz=2, over=0):
    """NBHD blocks of 16 tokens (block-ordered runs: the decoder's eight-token path) whose rows are 2 D elements apart and
    whose second head lies so far behind the first that the eighth row of a group ends exactly at the range."""
    st = 2 * D * esz
    sh = DESC_RANGE - D * esz - 7 * st + over * esz
    return RowsSpec(f"paged_head_stride_limit_e{esz}_over{over}", "NBHD", esz, BASE, INTERLEAVED, st, sh,
                    slot_table(16, False, T, [0, 5, 9, 2, 7, 11, 3]), 16, STRIDE_BLOCK)


def negative_stride(which, esz=2):
    """Refused: rows (or heads) that run downwards from a base 64 KiB further up."""
    st, sh = (-H * D * esz, D * esz) if which == "token" else (H * D * esz, -D * esz)
    return RowsSpec(f"negative_{which}_stride_e{esz}", "vllm", esz, BASE + 65536, INTERLEAVED, st, sh)


def _registry():
    specs = []
    for esz in (1, 2):
        for kind in ("NBHD", "NHBD"):
            for bs in (16, 12):
                for swapped in (False, True):
                    specs.append(paged_rows(kind, esz, bs, swapped))
        for swapped in (False, True):
            specs.append(paged_split(esz, swapped))
        for kind in ("vllm", "huggingface"):
            specs.append(dense(kind, esz))
        for over in (0, 1):
            specs.append(head_stride_limit(esz, over))
            specs.append(token_stride_limit(esz, over))
            specs.append(paged_head_stride_limit(esz, over))
        specs += [negative_stride("token", esz), negative_stride("head", esz)]
    return {s.name: s for s in specs}


REGISTRY = _registry()


def unsafe_addresses(spec, arena_bytes=ARENA_BYTES):
    """The safety property.  -> a list of findings (empty: safe): every true address, and every address with one offset
    reduced mod 2^32 or sign-extended from 32 bits, must lie in [0, arena_bytes)."""
    comps, extent = spec.components()
    names = list(comps)
    grids = np.ix_(*[np.asarray(comps[n], np.int64) for n in names])
    true = spec.base + sum(grids)
    bad = []

    def look(addr, what):
        lo, hi = int(addr.min()), int(addr.max()) + extent
        if lo < 0 or hi > arena_bytes:
            bad.append(f"{spec.name}: {what}: addresses {lo:#x} .. {hi:#x} leave the arena [0, {arena_bytes:#x})")

    look(true, "true")
    for n, g in zip(names, grids):
        look(true - g + mod32(g), f"{n} offset mod 2^32")
        look(true - g + sext32(g), f"{n} offset sign-extended from 32 bits")
    return bad


# ------------------------------------------------------------------ data in and out of the arena, window by window
def to_bytes(t):
    """torch [L, 2, T, H, D] of any element size -> numpy uint8 [L, 2, T, H, D * esz]."""
    t = t.contiguous().cpu()
    return t.view(torch.uint8).numpy().reshape(tuple(t.shape[:4]) + (t.shape[4] * t.element_size(),))


def expected_windows(offsets, data, fill=FILL, window=WINDOW):
    """(window starts [m], images uint8 [m, window]): the windows that hold a byte of the pieces (data[i] at byte offset
    offsets[i]), as they look when everything else holds the fill pattern."""
    offsets = np.asarray(offsets, np.int64).reshape(-1)
    if len(offsets) == 0:  # nothing may have been written at all
        return np.zeros(0, np.int64), np.zeros((0, window), np.uint8)
    data = np.ascontiguousarray(data, np.uint8).reshape(len(offsets), -1)
    byte_off = (offsets[:, None] + np.arange(data.shape[1], dtype=np.int64)).reshape(-1)
    wid = byte_off // window
    ids, inv = np.unique(wid, return_inverse=True)
    img = np.full((len(ids), window), fill, np.uint8)
    img[inv.reshape(-1), byte_off - wid * window] = data.reshape(-1)
    return ids * window, img


def write_windows(arena, starts, img, window=WINDOW):
    dev = torch.from_numpy(img).to(arena.device)
    for i, s in enumerate(starts.tolist()):
        arena[s:s + window].copy_(dev[i])


def read_windows(arena, starts, window=WINDOW):
    if len(starts) == 0:
        return np.zeros((0, window), np.uint8)
    return torch.stack([arena[s:s + window] for s in starts.tolist()]).cpu().numpy()


def restore_windows(arena, starts, fill=FILL, window=WINDOW):
    for s in starts.tolist():
        arena[s:s + window].fill_(fill)


def _words(fill):
    return int.from_bytes(bytes([fill] * 8), "little", signed=True)


def count_stray_words(arena, fill=FILL, slab=SLAB):
    """8-byte words of the arena that do not hold the fill pattern, counted slab by slab (one host wait)."""
    total = torch.zeros((), dtype=torch.int64, device=arena.device)
    for s in range(0, arena.numel(), slab):
        total += torch.count_nonzero(arena[s:s + slab].view(torch.int64) != _words(fill))
    return int(total)


def first_stray(arena, starts, fill=FILL, window=WINDOW, slab=SLAB):
    """Offset of the first byte outside the windows `starts` that does not hold the fill pattern, or None."""
    starts = np.asarray(starts, np.int64)
    for s in range(0, arena.numel(), slab):
        mask = arena[s:s + slab] != fill
        for w in starts[(starts >= s) & (starts < s + slab)].tolist():
            mask[w - s:w - s + window] = False
        if bool(mask.any()):
            return s + int(torch.argmax(mask.view(torch.uint8)))  # (the first of equal maxima)
    return None


def check_arena(arena, offsets, data, what="", fill=FILL, window=WINDOW, slab=SLAB):
    """The pieces hold their bytes and every other byte of the arena holds the fill pattern, or AssertionError naming the
    first wrong offset inside the expected windows and the first stray offset outside them.  -> the windows' starts."""
    starts, img = expected_windows(offsets, data, fill, window)
    got = read_windows(arena, starts, window)
    inside = int(np.count_nonzero(got.reshape(-1).view(np.int64) != _words(fill)))
    problems, missing = [], False
    if not np.array_equal(got, img):
        i, j = np.argwhere(got != img)[0]
        want, have = int(img[i, j]), int(got[i, j])
        if have == fill:
            missing = True
            kind = "an expected byte is missing, the fill pattern is still there"
        elif want == fill:
            kind = "a byte beside the expected rows was written"
        else:
            kind = "wrong value"
        problems.append(f"arena offset {int(starts[i]) + int(j):#x}: {kind} (expected {want:#04x}, found {have:#04x}; "
                        f"{int(np.count_nonzero(got != img))} bytes differ)")
    total = count_stray_words(arena, fill, slab)
    if total != inside:
        off = first_stray(arena, starts, fill, window, slab)
        note = ""
        for d, name in ((1 << 32, "2^32"), (1 << 31, "2^31")):
            if off is not None and (off // window * window + d) in set(starts.tolist()):
                note = f" = an expected window's address minus {name}"
        problems.append(f"{total - inside} 8-byte words outside the expected windows lost the fill pattern, first stray byte at "
                        f"arena offset {off:#x}{note}" if off is not None else "stray words counted but not found")
    elif missing:
        problems.append("no stray byte anywhere else: the store was dropped or never made")
    assert not problems, f"{what}: " + "; ".join(problems)
    return starts
