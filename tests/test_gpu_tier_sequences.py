"""The bounded local tiers under random operation sequences, at the level of the engine (LMCLocalBackend, tiering.py, the
arenas of storage_backend/arena.py): which region a decode reads, when it goes back, behind which events it is written again,
and what a key points at after a demotion, a transcode, a promotion or a second store.

Three configurations (tests/tier_sequences.py: make_engine), L = 2, H = 2, D = 64, bf16, chunks of 16 tokens:
  "hbm"    the coded HBM tier over a pinned tier: demotes by repack, promotes;
  "host"   the pinned tier alone: drops;
  "fixed"  the fixed-width tier with LMCACHE_AMD_FIXED_DEMOTE=1 and LMCACHE_AMD_FIXED_PROMOTE=1: demotes by transcode,
           promotes by the reverse transcode.
Thirteen prompts of 1 to 4 chunks with ragged tails, each with KV from a seed of its own; four pairs share a prefix of whole
chunks, tokens and KV (tier_sequences.POOL).  Every prompt's reference is computed once, per chunk, on the CPU by the oracle
(oracle_roundtrip) and serves all three configurations: the fixed-width model decodes to the coded one's bits
(test_gpu_fixed_model.py).  The group size of every prompt is measured once per configuration on a throwaway engine.

A sequence (tier_sequences.engine_ops) draws from: store blocking / queued / again (skip_existing=False), retrieve /
retrieve_layerwise / retrieve_into_paged ("NHBD", slots from 5 on), a decode begun by get_kv_range(..., jobs_out=jobs) and
finished 1 to 6 operations later (two in flight at most), set_capacity of either tier to None, 0, 1, 2.5 or 5 groups, drain.
The backend is drained behind four operations in five; the fifth races the worker thread.  The test's own calls run on a side
stream, the worker's on the default stream, so the events that fence a released region are what orders the two.

Behind EVERY operation:
  1. nothing raises, on the worker thread either (its log is read); a retrieve's mask is a prefix in whole chunks;
  2. the bits of the hit part equal the prompt's reference (torch.equal on int16 views); a paged retrieve wrote nothing else;
  3. a decode begun earlier and finished now equals its prompt's reference in every token it reported as hit.
Behind every DRAINED operation, under the tier lock:
  4. per bounded tier live_bytes <= budget, and reserved_bytes <= budget unless every slab still holds live bytes: an arena
     keeps a slab it took under a larger budget (or none) while something lives in it and takes no new one -- what
     PinnedArena's docstring says -- so "reserved <= budget" alone is not what the arenas promise once a budget shrinks;
     a slab that is one hole must have gone back;
  5. tier_stats()[tier]["live_bytes"] == the arena's live_bytes, less PinnedArena.cut_bytes: the tails an unbounded pinned
     arena could not cut off a pack because a store that overlapped it had its region behind it already;
  6. dict, _key_gid, _groups and the LRU agree: same keys, same gids, every group has a key of its own and is filed at its
     own size, the entry type of a key matches its group's tier, `groups` counts the distinct gids;
  7. liveness: behind a blocking store of a prompt that fits (Tiers.place on the measured sizes) that was stored WHOLE -- none
     of it was there, or skip_existing=False -- the prompt is a full hit; behind one that only added the rest to a prefix
     that was there, the rest is there (the new, smaller group may have pushed the prefix's own group out: that store
     cannot promise a full hit); while no budget is set, every prompt stored since is a full hit; and a retrieve of a
     prompt whose keys were all there is a full hit.
At the END of a sequence the decodes in flight are finished, both budgets go to 0 and the backend is drained:
  8. nothing is cached, every arena has 0 live bytes and every slab is one hole, every status word of the codec is back
     (the three pools of pinned buffers hold at least what they held: a buffer made while others were lent stays), and
     close() returns.
A group that had lost a key to a later store is never demoted (the rule _demote_group states), checked where it happens.

COVERAGE, summed over a configuration's default seeds and asserted (test_every_event_a_configuration_can_produce_occurred):
full hits from HBM, from a pinned pack and from a pinned single chunk, demotions, promotions, evictions, an oversize group
that was not cached, a key replaced in an older group that survives / that loses its last key, a group that could not be
demoted because it had lost a key, a decode finished after its group had been evicted or demoted -- each where the
configuration can produce it.

LMC_FUZZ_CASES (sequences per configuration, default 4) and LMC_FUZZ_SEED (first seed, default 0) widen the run.

WHAT THE SEQUENCES FOUND (the shortened sequences are the named cases at the end of the file):
  * bytes given back while no budget was set -- a key stored again -- stayed counted as live when a budget was set later:
    nothing could free them, the tier cached that much less than its budget (down to nothing) and its slab never went back;
  * a budget that shrank left a slab that was one hole reserved over the budget until the next free;
  * a promotion into an HBM arena that had the bytes and no hole large enough ended in "promotion failed" (ArenaFull) where
    a store and a demotion take the tier's LRU group out and try again.

Times on an MI355X: 0.04 to 0.14 s per sequence of 150 operations (0.4 s for the first one of the process, which warms the
codec up), 0.02 s for each named case, 4.3 s for the whole file with the references and the measured sizes.
"""
import os
import time
from collections import Counter

import pytest

from tests import tier_sequences as ts

pytestmark = pytest.mark.gpu

NSEEDS = int(os.environ.get("LMC_FUZZ_CASES", "4"))
SEED0 = int(os.environ.get("LMC_FUZZ_SEED", "0"))
NOPS = 150

# the events each configuration can produce (ts.EVENTS): the pinned tier alone has nothing above it and nothing to demote,
# the fixed-width tier's pinned groups are packs whatever their length
CAN = {"hbm": set(ts.EVENTS),
       "host": {"operations", "hit pack", "hit single", "evictions", "oversize", "replaced, group survives", "replaced, group goes",
                "decode outlived its group"},
       "fixed": set(ts.EVENTS) - {"hit single"}}
TOTALS = {c: Counter() for c in ts.CONFIGS}
RAN = {c: set() for c in ts.CONFIGS}


@pytest.fixture(scope="module")
def world(oracle):
    return ts.World(oracle)


@pytest.fixture
def fixed_switches(monkeypatch):
    monkeypatch.setenv("LMCACHE_AMD_FIXED_DEMOTE", "1")   # (both read when a backend is built)
    monkeypatch.setenv("LMCACHE_AMD_FIXED_PROMOTE", "1")


def _sequence(world, config, seed):
    """One default sequence, once per process: what it counted goes into TOTALS."""
    if seed in RAN[config]:
        return
    world.sizes(config)
    t0 = time.perf_counter()
    seen = ts.replay(config, ts.engine_ops(config, seed, NOPS), world, tag=f"seed {seed}")
    print(f"\n{config} seed {seed}: {time.perf_counter() - t0:.2f} s, {dict(seen)}")
    RAN[config].add(seed)
    TOTALS[config].update(seen)


@pytest.mark.parametrize("seed", range(SEED0, SEED0 + NSEEDS))
@pytest.mark.parametrize("config", ts.CONFIGS)
def test_a_random_sequence_leaves_every_prompt_its_own_bits_and_every_byte_accounted_for(world, fixed_switches, config, seed):
    _sequence(world, config, seed)


@pytest.mark.parametrize("config", ts.CONFIGS)
def test_every_event_a_configuration_can_produce_occurred(world, fixed_switches, config):
    """Sums what the configuration's sequences counted (they have run already in the file's order; one that has not, because
    this test was selected alone, runs here)."""
    for seed in range(SEED0, SEED0 + NSEEDS):
        _sequence(world, config, seed)
    total = TOTALS[config]
    assert total["operations"] == NSEEDS * NOPS
    print(f"\n{config} total over seeds {SEED0}..{SEED0 + NSEEDS - 1}: {dict(total)}")
    missing = sorted(e for e in CAN[config] if total[e] == 0)
    assert not missing, f"{config}: never happened in seeds {SEED0}..{SEED0 + NSEEDS - 1}: {missing}; counted {dict(total)}"


# ---- the shortened sequences of what the random ones found, kept as plain cases ---------------------------------------------
def test_bytes_given_back_before_a_budget_was_set_are_free_behind_it(world):
    """Prompt 0 stored twice with no budget: the first store's blobs go back to a bump allocator, which only counts them.  A
    budget of 2.5 groups set afterwards used to find those bytes live for good: 1.5 groups were left, then less and less."""
    ops = [("store", 0, "blocking", True), ("store", 0, "again", True), ("store", 0, "again", True),
           ("cap", "hbm", 2.5, True), ("store", 12, "blocking", True), ("retrieve", 0, "dense", True),
           ("retrieve", 12, "layerwise", True), ("cap", "hbm", 1, True), ("store", 0, "again", True),
           ("retrieve", 0, "paged", True)]
    seen = ts.replay("hbm", ops, world, tag="regression")
    # (a group of three keys that is stored again loses two keys and survives, then the third and goes)
    assert (seen["hit hbm"], seen["replaced, group survives"], seen["replaced, group goes"]) == (3, 4, 2)


def test_the_same_on_the_pinned_tier_where_the_bytes_are_a_pack(world):
    ops = [("store", 6, "blocking", True), ("store", 7, "again", True), ("store", 7, "again", True),
           ("cap", "pinned", 5, True), ("store", 10, "blocking", True), ("retrieve", 7, "dense", True),
           ("retrieve", 10, "dense", True), ("cap", "pinned", 2.5, True), ("retrieve", 10, "layerwise", True)]
    seen = ts.replay("host", ops, world, tag="regression")
    assert (seen["hit pack"], seen["replaced, group survives"], seen["replaced, group goes"]) == (3, 4, 2)


# (the first 92 operations of engine_ops("hbm", 5, 150), as they were when the sequence failed)
PROMOTION_INTO_A_FRAGMENTED_ARENA = [
    ('store', 8, 'blocking', True), ('store', 10, 'blocking', True), ('store', 10, 'again', True), ('store', 6, 'queued',
    True), ('store', 9, 'again', True), ('retrieve', 3, 'dense', True), ('begin', 9, True), ('store', 1, 'blocking',
    False), ('cap', 'hbm', 5, True), ('retrieve', 6, 'dense', True), ('finish', 1, True), ('retrieve', 9, 'paged', True),
    ('retrieve', 10, 'dense', True), ('cap', 'pinned', 0, True), ('retrieve', 5, 'dense', True), ('retrieve', 1, 'paged',
    True), ('store', 6, 'queued', False), ('retrieve', 0, 'dense', True), ('cap', 'pinned', 5, True), ('store', 10,
    'blocking', True), ('store', 0, 'blocking', False), ('store', 6, 'blocking', True), ('store', 7, 'again', True),
    ('store', 7, 'again', True), ('store', 7, 'again', True), ('store', 1, 'blocking', False), ('begin', 1, True),
    ('retrieve', 7, 'dense', True), ('store', 8, 'queued', True), ('store', 9, 'blocking', True), ('store', 9, 'queued',
    True), ('cap', 'hbm', 1, True), ('finish', 0, False), ('drain', True), ('store', 5, 'queued', True), ('store', 5,
    'blocking', True), ('begin', 5, True), ('retrieve', 5, 'dense', True), ('store', 11, 'again', True), ('store', 3,
    'blocking', True), ('finish', 0, True), ('retrieve', 6, 'paged', True), ('begin', 11, True), ('cap', 'hbm', 1, True),
    ('store', 0, 'blocking', False), ('store', 4, 'queued', True), ('cap', 'pinned', 1, True), ('store', 5, 'again',
    False), ('finish', 0, True), ('retrieve', 4, 'paged', True), ('store', 4, 'again', False), ('store', 9, 'again',
    True), ('cap', 'hbm', 5, True), ('store', 4, 'again', True), ('retrieve', 9, 'paged', True), ('retrieve', 12, 'dense',
    True), ('store', 5, 'blocking', False), ('drain', True), ('cap', 'hbm', 0, False), ('retrieve', 4, 'dense', True),
    ('retrieve', 1, 'dense', True), ('cap', 'hbm', 5, True), ('cap', 'pinned', 5, True), ('retrieve', 4, 'layerwise',
    True), ('retrieve', 5, 'paged', True), ('retrieve', 1, 'dense', True), ('begin', 11, False), ('finish', 0, True),
    ('retrieve', 11, 'layerwise', True), ('retrieve', 6, 'dense', True), ('begin', 6, False), ('retrieve', 6, 'dense',
    True), ('retrieve', 11, 'layerwise', True), ('cap', 'hbm', 1, True), ('cap', 'hbm', 0, True), ('finish', 0, True),
    ('cap', 'hbm', 2.5, True), ('store', 9, 'again', True), ('retrieve', 9, 'paged', False), ('store', 5, 'again', True),
    ('store', 3, 'blocking', True), ('retrieve', 5, 'dense', True), ('store', 0, 'queued', True), ('retrieve', 4,
    'layerwise', True), ('begin', 0, True), ('store', 2, 'blocking', True), ('retrieve', 12, 'dense', True), ('retrieve',
    12, 'paged', True), ('store', 5, 'blocking', False), ('finish', 0, True), ('begin', 2, True), ('retrieve', 5, 'dense',
    True)]


def test_a_promotion_into_a_fragmented_hbm_arena_makes_its_own_room(world):
    """The byte count allows the promoted group, no hole of the HBM arena is large enough: _promote_group used to end in
    "promotion failed" (ArenaFull, logged with its traceback) where a store and a demotion take the tier's LRU group out
    and try again.  It does the same now; the log stays clean (replay reads it) and the group comes up."""
    seen = ts.replay("hbm", PROMOTION_INTO_A_FRAGMENTED_ARENA, world, tag="regression")
    assert seen["promotions"] >= 1
