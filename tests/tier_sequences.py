"""Random operation sequences over the bounded local tiers: the generators, the log format and `replay`.

Two levels share this file:

  host_ops(seed, n)          operations over Tiers / GroupLRU with fake movers (tests/test_tiering_sequences_host.py holds
                             the brute-force model they are checked against);
  engine_ops(config, seed, n), replay(config, ops, world)
                             operations over a whole LMCacheEngine on the GPU (tests/test_gpu_tier_sequences.py).

THE LOG FORMAT.  An operation is a plain tuple whose last element says whether the backend is drained behind it, and a
sequence is a list of them, so that `repr(ops)` pasted into `replay(config, ops, world)` runs the same sequence again and a
failing one can be cut down by hand:

  ("store", p, how, drained)       how: "blocking", "queued" (blocking=False) or "again" (skip_existing=False, blocking)
  ("retrieve", p, form, drained)   form: "dense" (retrieve), "layerwise" (retrieve_layerwise, layers_per_launch=1) or "paged"
                                   (retrieve_into_paged into an "NHBD" cache, slots from 5 on)
  ("begin", p, drained)            get_kv_range(..., layers_per_launch=1, jobs_out=jobs) into a destination of its own
  ("finish", k, drained)           finish_decode of the k-th oldest decode in flight (modulo how many there are)
  ("cap", tier, level, drained)    set_capacity: `tier`'s budget becomes None, or `level` groups of the measured size
  ("drain", drained)

p is an index into POOL.  Every failure message of replay() carries the configuration, the index of the failing operation
and the operations up to it.
"""
import logging
import random
from collections import Counter

# ---------------------------------------------------------------------------------------------------------------------
# host level
# ---------------------------------------------------------------------------------------------------------------------
HOST_KINDS = ("add", "store", "touch", "touch_chain", "resize", "remove", "budget", "make_room", "take_lru", "enforce",
              "promote")
_HOST_WEIGHTS = (10, 14, 8, 12, 6, 4, 8, 10, 8, 8, 8)
UNIT = 160  # a "group size" of the host sequences (bytes; multiples of 16 as everything the arenas hand out)


def host_ops(seed: int, n: int = 300) -> list:
    """n operations over Tiers / GroupLRU.  Group ids are drawn from a small range, so that most operations meet a group
    that exists and some meet one that has gone (the classes under test take both)."""
    rng = random.Random(seed)
    ops, next_gid = [], 0

    def some_gid():
        return rng.randrange(max(1, next_gid)) if rng.random() < 0.9 else next_gid + 3

    def keep():
        return [some_gid() for _ in range(rng.choice((0, 0, 1, 1, 2, 3)))]

    for _ in range(n):
        kind = rng.choices(HOST_KINDS, _HOST_WEIGHTS)[0]
        if kind in ("add", "store"):
            ops.append((kind, next_gid, 16 * rng.randint(1, 30)))
            next_gid += 1
        elif kind == "touch":
            ops.append((kind, some_gid()))
        elif kind == "touch_chain":
            chain = [some_gid() for _ in range(rng.randint(1, 4))]
            ops.append((kind, [g for g in chain for _ in range(rng.randint(1, 3))]))  # several chunks per group
        elif kind == "resize":
            ops.append((kind, some_gid(), 16 * rng.randint(0, 20)))
        elif kind == "remove":
            ops.append((kind, some_gid()))
        elif kind == "budget":
            ops.append((kind, rng.choice(("hbm", "pinned")), rng.choice((None, 0, UNIT, 2 * UNIT + 80, 5 * UNIT, 5 * UNIT))))
        elif kind == "make_room":
            ops.append((kind, rng.choice(("hbm", "pinned")), 16 * rng.randint(0, 40), keep()))
        elif kind == "take_lru":
            ops.append((kind, rng.choice(("hbm", "pinned")), keep()))
        elif kind == "enforce":
            ops.append((kind, keep()))
        else:
            ops.append((kind, some_gid()))
    return ops


# ---------------------------------------------------------------------------------------------------------------------
# engine level
# ---------------------------------------------------------------------------------------------------------------------
CONFIGS = ("hbm", "host", "fixed")
CS, L_, H_, D_, BS = 16, 2, 2, 64, 16
DEV = "cuda:0"
MODEL = "mistralai/Mistral-7B-Instruct-v0.2"

# (tokens, parent, shared whole chunks): a prompt with a parent has the parent's first `shared` chunks of tokens and the
# parent's KV on them, then a continuation of its own.  Storing the child whole takes those keys out of the parent's group:
# 1 and 3 leave their parent a tail, 5 and 7 take every key their parent has.
POOL = ((40, None, 0), (56, 0, 2), (24, None, 0), (64, 2, 1), (16, None, 0), (40, 4, 1), (32, None, 0), (56, 6, 2),
        (16, None, 0), (24, None, 0), (56, None, 0), (64, None, 0), (40, None, 0))
UNIT_PROMPT = 0            # budgets are multiples of this prompt's measured group size (three chunks: 16, 16, 8 tokens)
LEVELS = (None, 0, 1, 2.5, 5)
_LEVEL_WEIGHTS = (2, 1, 3, 5, 3)
ENGINE_KINDS = ("store blocking", "store queued", "store again", "retrieve dense", "retrieve layerwise", "retrieve paged",
                "begin", "finish", "cap", "drain")
_ENGINE_WEIGHTS = {"store blocking": 14, "store queued": 8, "store again": 14, "retrieve dense": 14, "retrieve layerwise": 8,
                   "retrieve paged": 8, "begin": 9, "cap": 13, "drain": 3}


def kind_of(op) -> str:
    return f"{op[0]} {op[2]}" if op[0] in ("store", "retrieve") else op[0]


def _relatives(p: int) -> list:
    """p, its parent and its children."""
    out = [p] + [q for q, (_, parent, _) in enumerate(POOL) if parent == p]
    if POOL[p][1] is not None:
        out.append(POOL[p][1])
    return out


def engine_ops(config: str, seed: int, n: int = 150) -> list:
    """About n operations for `config`, every kind at least once.  A decode that is begun is finished 1 to 6 operations later,
    at most two are in flight; about one operation in five is not drained behind (never two in a row, so that at most one
    operation races the worker's queue); "store again" prefers a prompt that was stored lately, or a relative of it."""
    assert config in CONFIGS
    rng = random.Random(f"{config}/{seed}")
    tiers = ("pinned",) if config == "host" else ("hbm", "pinned")
    for _ in range(100):
        ops, due, recent, raced = [], [], [], False
        while len(ops) < n:
            drained = raced or rng.random() >= 0.2
            raced = not drained
            if due and due[0] <= len(ops):
                due.pop(0)
                ops.append(("finish", rng.randrange(2), drained))
                continue
            names = [k for k in _ENGINE_WEIGHTS if k != "begin" or len(due) < 2]
            kind = rng.choices(names, [_ENGINE_WEIGHTS[k] for k in names])[0]
            if kind.startswith("store"):
                how = kind.split()[1]
                p = rng.randrange(len(POOL))
                if how == "again" and recent and rng.random() < 0.8:
                    p = rng.choice(_relatives(rng.choice(recent)))
                recent = (recent + [p])[-3:]
                ops.append(("store", p, how, drained))
            elif kind.startswith("retrieve"):
                p = rng.choice(recent) if recent and rng.random() < 0.5 else rng.randrange(len(POOL))
                ops.append(("retrieve", p, kind.split()[1], drained))
            elif kind == "begin":
                p = rng.choice(recent) if recent and rng.random() < 0.7 else rng.randrange(len(POOL))
                ops.append(("begin", p, drained))
                due.append(len(ops) + rng.randint(0, 5))
                due.sort()
            elif kind == "cap":
                ops.append(("cap", rng.choice(tiers), rng.choices(LEVELS, _LEVEL_WEIGHTS)[0], drained))
            else:
                ops.append(("drain", True))
        if {kind_of(op) for op in ops} >= set(ENGINE_KINDS):
            return ops
    raise AssertionError("no sequence with every kind of operation")


class World:
    """What every sequence shares and nothing changes: the prompts, their KV, the CPU reference of each prompt and the
    measured group sizes per configuration."""

    def __init__(self, oracle):
        import torch
        from tests.test_gpu_engine import oracle_roundtrip
        self.tokens, self.kv, self.ref, self._sizes = [], [], [], {}
        for p, (n, parent, shared) in enumerate(POOL):
            g = torch.Generator().manual_seed(4000 + p)          # every prompt's tokens and KV from its own seed
            tokens = torch.randint(0, 10000, (n,), generator=g) + 20000 * p
            kv = [[torch.randn((n, H_, D_), generator=g).to(torch.bfloat16) for _ in range(2)] for _ in range(L_)]
            if parent is not None:
                m = shared * CS
                tokens[:m] = self.tokens[parent][:m].cpu()
                for l in range(L_):
                    for j in range(2):
                        kv[l][j][:m] = self.kv[parent][l][j][:m].cpu()
            kv = tuple((k, v) for k, v in kv)
            # the reference: per chunk, on the CPU, by the oracle -- never by the engine under test
            parts = [oracle_roundtrip(oracle, tuple((k[t:t + CS], v[t:t + CS]) for k, v in kv), "vllm", MODEL, torch.bfloat16)
                     for t in range(0, n, CS)]
            self.ref.append(torch.cat(parts, dim=2).contiguous().view(torch.int16).to(DEV))
            self.tokens.append(tokens.to(DEV))
            self.kv.append(tuple((k.to(DEV), v.to(DEV)) for k, v in kv))
        torch.cuda.synchronize()

    def sizes(self, config: str) -> list:
        """Per prompt (bytes of its whole group in the tier a store lands in, bytes once it lies in the pinned tier below
        -- for "fixed" the bound room is made for, which is what place() compares), measured once on a throwaway engine."""
        if config not in self._sizes:
            import torch
            from lmcache_amd import native
            eng = make_engine(config)
            be = eng.engine_
            out = []
            try:
                for p in range(len(POOL)):
                    eng.store(self.tokens[p], self.kv[p], skip_existing=False)
                    st = be.tier_stats()
                    if config == "host":
                        out.append((st["pinned"]["live_bytes"], st["pinned"]["live_bytes"]))
                    else:
                        top = st["hbm"]["live_bytes"]
                        be.set_capacity(hbm_bytes=0, pinned_bytes=1 << 30)
                        low = be.tier_stats()["pinned"]["live_bytes"]
                        if config == "fixed":
                            low = native.r16(native.pack_bound((POOL[p][0] + CS - 1) // CS, L_, CS, H_, D_))
                        out.append((top, low))
                    assert min(out[-1]) > 0
                    be.set_capacity(hbm_bytes=0, pinned_bytes=0)
                    be.drain()
                    assert not be.dict
                    be.set_capacity(None, None)
            finally:
                torch.cuda.synchronize()
                eng.close()
            self._sizes[config] = out
        return self._sizes[config]


def make_engine(config: str):
    """The engine of a configuration.  "fixed" reads LMCACHE_AMD_FIXED_DEMOTE / LMCACHE_AMD_FIXED_PROMOTE here: the caller
    has set them."""
    from lmcache_amd.cache_engine import LMCacheEngine
    from lmcache_amd.config import LMCacheEngineConfig
    from tests.test_gpu_engine import dumb_metadata, make_cfg
    if config == "fixed":
        cfg = LMCacheEngineConfig.from_legacy(chunk_size=CS, backend="cuda", local_serde="cachegen-fixed")
    else:
        cfg = make_cfg({"hbm": "cachegen-hbm", "host": "cachegen-host"}[config], CS)
    eng = LMCacheEngine(cfg, dumb_metadata("vllm", MODEL))
    if config == "fixed":
        assert eng.engine_.fixed_demotes and eng.engine_.fixed_promotes, "set LMCACHE_AMD_FIXED_DEMOTE / _PROMOTE first"
    return eng


# what replay() counts (the coverage conditions of test_gpu_tier_sequences.py are sums of these over a configuration's seeds)
EVENTS = ("operations", "hit hbm", "hit pack", "hit single", "demotions", "promotions", "evictions", "oversize",
          "replaced, group survives", "replaced, group goes", "undemotable", "decode outlived its group")


class SequenceFailed(AssertionError):
    """A check of replay() that did not hold; the message says where and how to run it again."""


def replay(config: str, ops: list, world: World, tag: str = "") -> Counter:
    """Run `ops` (the log format above) on a fresh engine of `config` with every check of test_gpu_tier_sequences.py's
    docstring behind every operation and at the end -> what happened, counted (EVENTS)."""
    import torch
    from lmcache_amd import native
    from lmcache_amd.storage_backend.local_backend import _DevChunk, _HostChunk, _PackChunk
    from tests.test_gpu_codec import _words_out

    sizes = world.sizes(config)
    unit = sizes[UNIT_PROMPT]
    tiered_cfg = config != "host"
    eng = make_engine(config)
    be = eng.engine_
    codec = be._codec()
    seen = Counter()
    state = {"i": -1, "op": None}

    def fail(msg):
        i = state["i"]
        raise SequenceFailed(f"{config} {tag}: operation {i} {state['op']!r}: {msg}\n"
                             f"replay({config!r}, {ops[:i + 1]!r}, world)")

    def check(cond, msg):
        if not cond:
            fail(msg() if callable(msg) else msg)

    # ---- what is counted from inside: thin wrappers that change nothing
    real_demote, real_replaced, real_not_cached = be._tiers._demote, be._release_replaced, be._not_cached

    problems = []  # what was seen where raising would be swallowed (the worker thread): looked at behind every operation

    def demote(gid):
        g = be._groups[gid]
        lost = len(be._own_keys(g)) != len(g.keys)
        ok = real_demote(gid)
        if lost:
            seen["undemotable"] += 1
            if ok:
                problems.append(f"group {gid} had lost a key to a later store and was demoted all the same")
        return ok

    class Errors(logging.Handler):
        """1. nothing raises -- on the worker thread either, where an exception ends in the log."""

        def emit(self, record):
            text = record.getMessage()
            if record.levelno >= logging.ERROR or ("demotion failed" in text and "ArenaFull" not in text):
                if record.exc_info and record.exc_info[1] is not None:
                    text += f" ({type(record.exc_info[1]).__name__}: {record.exc_info[1]})"
                problems.append("logged: " + text)

    errors = Errors(level=logging.WARNING)
    logging.getLogger("lmcache_amd").addHandler(errors)

    def replaced(old_gid, old_e):
        known = old_gid in be._groups
        real_replaced(old_gid, old_e)
        if known:
            seen["replaced, group survives" if old_gid in be._groups else "replaced, group goes"] += 1

    def not_cached(nbytes):
        seen["oversize"] += 1
        real_not_cached(nbytes)

    if be._tiers._demote is not None:
        be._tiers._demote = demote
    be._release_replaced, be._not_cached = replaced, not_cached

    keys = [[eng._make_key(h, "vllm") for h in eng._prefix_hashes_of(t)] for t in world.tokens]
    budget = {"hbm": None, "pinned": None}
    inflight, since_unbounded = [], set()
    side = torch.cuda.Stream()  # (the worker thread queues on the default stream: the fences between the two are real ones)
    words = None

    def fits(p):
        """Whether a store of the WHOLE prompt p as one group is kept under the budgets of the moment (Tiers.place)."""
        top, low = sizes[p]
        if not tiered_cfg:
            return budget["pinned"] is None or top <= budget["pinned"]
        if budget["hbm"] is None or top <= budget["hbm"]:
            return True
        return budget["pinned"] is not None and (low if config == "fixed" else top) <= budget["pinned"]

    def hit_bits(p, got_bits, hits, what):
        check(torch.equal(got_bits, world.ref[p][:, :, :hits]),
              lambda: f"{what} of prompt {p}: {int((got_bits != world.ref[p][:, :, :hits]).sum())} of {got_bits.numel()} "
                      f"16-bit words of the {hits} hit tokens differ from the reference")

    def prefix_mask(p, mask):
        n = POOL[p][0]
        hits = int(mask.sum())
        check(mask.numel() == n and bool(mask[:hits].all()) and (hits % CS == 0 or hits == n),
              f"the mask of prompt {p} is no prefix in whole chunks: {mask.tolist()}")
        return hits

    def where(p):
        """The tiers' view of prompt p before a hit: "hbm", "pack", "single", or None (not whole, or mixed)."""
        es = [be.dict.get(k) for k in keys[p]]
        if any(e is None for e in es):
            return None
        for name, cls in (("hbm", _DevChunk), ("pack", _PackChunk), ("single", _HostChunk)):
            if all(isinstance(e, cls) for e in es):
                return name
        return None

    def finish(entry):
        """3. a decode begun earlier: every token it reported as hit equals the reference, whatever became of its group."""
        p, out, jobs, got, read = entry
        for job_codec, job in jobs:
            job_codec.finish_decode(job)
        side.synchronize()
        hits = min(got * CS, POOL[p][0])
        bits = out.view(torch.int16)
        if hits:
            hit_bits(p, bits[:, :, :hits], hits, "decode begun earlier")
        check(not bool(bits[:, :, hits:].any()), f"the decode of prompt {p} wrote behind its {hits} hit tokens")
        with be._tier_lock:
            if any(g not in be._groups or be._lru.tier_of(g) != t for g, t in read.items()):
                seen["decode outlived its group"] += 1

    def structure():
        """Checks 4 - 7 (the module docstring of test_gpu_tier_sequences.py), under the tier lock, nothing queued."""
        with be._tier_lock:
            st = be.tier_stats()
            for tier, arena in (("hbm", be.dev_arena), ("pinned", be.host_arena)):
                live, b = st[tier]["live_bytes"], st[tier]["budget"]
                check(b == budget[tier], f"{tier}: budget {b}, set to {budget[tier]}")
                if arena is None:
                    check(live == 0, f"{tier}: {live} live bytes and no arena")
                    continue
                # bytes of the arena that belong to no group: the tails an UNBOUNDED pinned arena could not cut off a pack
                # because another allocation lay behind it already (PinnedArena.cut_bytes; holes once it is bounded)
                cut = getattr(arena, "cut_bytes", 0)
                check(arena.live_bytes - cut == live, f"{tier}: the groups hold {live} bytes, the arena has {arena.live_bytes} "
                                                      f"live ({cut} of them cut tails)")
                if b is not None:
                    check(live <= b, f"{tier}: {live} live bytes over the budget of {b}")
                    fl = arena._fl
                    # reserved bytes: within the budget too, but for slabs taken under a larger budget (or none) that still
                    # hold live bytes -- the arena keeps those and takes no new one (PinnedArena's docstring); one that is a
                    # single hole must have gone back
                    check(st[tier]["reserved_bytes"] <= b or not any(fl.is_empty(s) for s in fl.slabs),
                          f"{tier}: {st[tier]['reserved_bytes']} bytes reserved over the budget of {b} with an empty slab among them")
            gids = set(be._key_gid.values())
            filed = {g for t in ("hbm", "pinned") for g in be._lru.groups(t)}
            check(set(be.dict) == set(be._key_gid), "dict and _key_gid hold different keys")
            check(gids == set(be._groups) == filed, f"gids of the keys {sorted(gids)}, groups {sorted(be._groups)}, LRU {sorted(filed)}")
            check(st["hbm"]["groups"] + st["pinned"]["groups"] == len(gids), "tier_stats counts other groups")
            for gid, g in be._groups.items():
                own = be._own_keys(g)
                tier = be._lru.tier_of(gid)
                check(bool(own), f"group {gid} has no key of its own")
                check(be._lru.nbytes(gid) == g.nbytes, f"group {gid}: {g.nbytes} bytes, filed at {be._lru.nbytes(gid)}")
                for k in own:
                    up = isinstance(be.dict[k], (_DevChunk, torch.Tensor))
                    check(up == (tier == "hbm"), f"group {gid} is filed in {tier}, a key of it is a {type(be.dict[k]).__name__}")
            if all(budget[t] is None for t in (("hbm", "pinned") if tiered_cfg else ("pinned",))):
                for p in sorted(since_unbounded):
                    check(be.contains_prefix(list(keys[p])) == len(keys[p]), f"no budget is set and prompt {p}, stored since, is no full hit")

    try:
        with torch.cuda.stream(side):
            words = _words_out(codec)
            quiet = True  # nothing queued on the worker: the state is a function of the operations so far
            for i, op in enumerate(ops):
                state["i"], state["op"] = i, op
                kind, drained = op[0], op[-1]
                seen["operations"] += 1
                try:
                    if kind == "store":
                        p, how = op[1], op[2]
                        present = be.contains_prefix(list(keys[p]))
                        if how == "queued":
                            eng.store(world.tokens[p], world.kv[p], blocking=False)
                        else:
                            eng.store(world.tokens[p], world.kv[p], skip_existing=how != "again")
                        if all(b is None for b in budget.values()):
                            since_unbounded.add(p)
                        if how != "queued" and quiet and fits(p):
                            # liveness.  A store of the whole prompt (none of it was there, or skip_existing=False) is one
                            # group of the measured size: a full hit.  A store behind a prefix that was there files the rest
                            # as a smaller group and may push that prefix's group out to make room: the rest is there.
                            first = 0 if how == "again" else present
                            have = [be.contains(k) for k in keys[p]]
                            check(all(have[first:]), f"prompt {p} fits its tier and chunks {first}.. of it are not all there after "
                                                     f"a blocking store: {have}")
                    elif kind == "retrieve":
                        p, form = op[1], op[2]
                        lies = where(p) if quiet else None
                        if form == "dense":
                            kv, mask = eng.retrieve(world.tokens[p])
                        elif form == "layerwise":
                            lw = eng.retrieve_layerwise(world.tokens[p], layers_per_launch=1)
                            for l in range(L_):
                                lw.wait_layer(l)
                            lw.finish()
                            kv, mask = lw.kv, lw.ret_mask
                        else:
                            n = POOL[p][0]
                            nb = (n + 5 + BS - 1) // BS + 1
                            caches = [torch.zeros((2, nb, H_, BS, D_), dtype=torch.bfloat16, device=DEV) for _ in range(L_)]
                            slots = (torch.arange(n, dtype=torch.int64) + 5).to(DEV)
                            mask = eng.retrieve_into_paged(world.tokens[p], caches, slots, BS, "NHBD")
                        hits = prefix_mask(p, mask)
                        if form == "paged":
                            side.synchronize()
                            rows = torch.stack(caches).permute(0, 1, 2, 4, 3, 5).reshape(L_, 2, -1, H_, D_).view(torch.int16)
                            if hits:
                                hit_bits(p, rows[:, :, 5:5 + hits].contiguous(), hits, "paged retrieve")
                            rows[:, :, 5:5 + hits] = 0
                            check(not bool(rows.any()), f"paged retrieve of prompt {p} wrote outside the slots of its {hits} hit tokens")
                        elif hits:
                            got = torch.stack([torch.stack(l) for l in kv]).contiguous().view(torch.int16)
                            check(got.shape[2] == hits, f"{hits} tokens in the mask, {got.shape[2]} returned")
                            hit_bits(p, got, hits, f"{form} retrieve")
                        else:
                            check(len(kv) == 0, "a miss that returns KV")
                        if lies is not None:
                            check(hits == POOL[p][0], f"every key of prompt {p} was there ({lies}) and the retrieve hit {hits} tokens")
                            seen[f"hit {lies}"] += 1
                    elif kind == "begin":
                        p = op[1]
                        out = torch.zeros((L_, 2, POOL[p][0], H_, D_), dtype=torch.bfloat16, device=DEV)
                        jobs = []
                        with be._tier_lock:
                            read = {be._key_gid[k] for k in keys[p][:be.contains_prefix(list(keys[p]))]}
                            read = {g: be._lru.tier_of(g) for g in read}
                            got = be.get_kv_range(list(keys[p]), native.KVLayout.from_chunk(out, "vllm"), "vllm", 0, CS,
                                                  layers_per_launch=1, jobs_out=jobs)
                        inflight.append((p, out, jobs, got, read))
                    elif kind == "finish":
                        if inflight:
                            finish(inflight.pop(op[1] % len(inflight)))
                    elif kind == "cap":
                        tier, level = op[1], op[2]
                        budget[tier] = None if level is None else int(level * unit[0 if tier == "hbm" or not tiered_cfg else 1])
                        if any(b is not None for b in budget.values()):
                            since_unbounded.clear()
                        be.set_capacity(hbm_bytes=budget["hbm"], pinned_bytes=budget["pinned"])
                    else:
                        check(kind == "drain", "an unknown kind of operation")
                        be.drain()
                    if drained:
                        be.drain()
                        structure()
                    quiet = bool(drained)
                    check(not problems, lambda: "; ".join(problems))
                except SequenceFailed:
                    raise
                except Exception as exc:  # 1. nothing raises (an assertion of the product's own included)
                    fail(f"raised {type(exc).__name__}: {exc}")
            # ---- 8. the end: everything goes, and everything comes back
            state["i"], state["op"] = len(ops) - 1, "the end of the sequence"
            while inflight:
                finish(inflight.pop(0))
            budget["hbm"] = budget["pinned"] = 0
            be.set_capacity(hbm_bytes=0, pinned_bytes=0)
            be.drain()
            structure()
            check(not be.dict and not be._groups, "budgets of 0 and something is still cached")
            for name, arena in (("HBM", be.dev_arena), ("pinned", be.host_arena)):
                if arena is not None:
                    fl = arena._fl
                    check(arena.live_bytes == 0, f"the {name} arena still has {arena.live_bytes} live bytes")
                    check(all(fl.is_empty(s) for s in fl.slabs), f"a slab of the {name} arena is not one hole")
            side.synchronize()
            after = _words_out(codec)
            # every job has given its status word back; the three pools of pinned buffers hold every buffer again, and may
            # have grown by the buffers that were made while others were lent
            check(after[0] == words[0] and all(a >= b for a, b in zip(after[1:], words[1:])),
                  f"the codec's words: {words} before the first operation, {after} now")
        st = be.tier_stats()
        for name in ("demotions", "promotions", "evictions"):
            seen[name] = st[name]
        check(not problems, lambda: "; ".join(problems))
    finally:
        logging.getLogger("lmcache_amd").removeHandler(errors)
        torch.cuda.synchronize()
        eng.close()   # (returns: the worker thread ends)
    return seen
