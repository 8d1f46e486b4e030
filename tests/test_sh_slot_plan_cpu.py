"""The slot policy of the shared-LTI backward pass's kept record streams (sh_slot_plan in csrc/back_pass_sh.hip), through the unlisted debug
hook ddp_sh_slot_plan — the function the grouping kernel calls, compiled for the host: 10 000 random states of the 16 slots (keys, empty /
complete, launch of last use) and 1..16 group keys, some of them keys of the slots."""
import ctypes as C

import numpy as np

SLOTS = 16


def _plan():
    from ddp_amd import _lib
    f = _lib.lib().ddp_sh_slot_plan
    u64p, ip = C.POINTER(C.c_uint64), C.POINTER(C.c_int)
    f.argtypes = [u64p, ip, ip, C.c_int, u64p, ip]
    f.restype = C.c_int

    def plan(skey, sstate, sused, gkey):
        skey, gkey = np.ascontiguousarray(skey, np.uint64), np.ascontiguousarray(gkey, np.uint64)
        sstate, sused = np.ascontiguousarray(sstate, np.intc), np.ascontiguousarray(sused, np.intc)
        gslot = np.full(SLOTS, -7, np.intc)
        hits = f(skey.ctypes.data_as(u64p), sstate.ctypes.data_as(ip), sused.ctypes.data_as(ip), len(gkey), gkey.ctypes.data_as(u64p), gslot.ctypes.data_as(ip))
        assert hits >= 0
        return gslot[: len(gkey)], [(hits >> g) & 1 == 1 for g in range(len(gkey))]
    return plan


def test_header_does_not_list_the_hook():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert "ddp_sh_slot_plan" not in open(os.path.join(root, "include", "ddp_amd.h")).read()


def test_every_slot_empty_gives_group_g_slot_g():
    """the layout of a launch without reuse"""
    plan = _plan()
    for G in range(1, SLOTS + 1):
        gslot, hit = plan(np.zeros(SLOTS), np.zeros(SLOTS), np.arange(SLOTS), np.arange(100, 100 + G))
        assert list(gslot) == list(range(G)) and not any(hit)


def test_random_states():
    plan = _plan()
    rng = np.random.default_rng(2025)
    seen_hit = seen_evict = seen_mixed = 0
    for _ in range(10000):
        pool = rng.permutation(40).astype(np.uint64) + 1            # λ bit patterns stand-ins
        sstate = (rng.random(SLOTS) < rng.choice([0.2, 0.6, 1.0])).astype(np.intc)
        skey = np.zeros(SLOTS, np.uint64)
        full = np.flatnonzero(sstate == 1)
        skey[full] = pool[: len(full)]                              # complete slots hold distinct keys
        for s in np.flatnonzero(sstate == 0):                       # an empty slot may carry any key, one of a complete slot included
            skey[s] = pool[rng.integers(0, 24)]
        sused = rng.integers(0, 6 if rng.random() < 0.3 else 1000, SLOTS).astype(np.intc)      # (with ties among the ages)
        G = int(rng.integers(1, SLOTS + 1))
        gkey = rng.permutation(pool[: max(G, int(rng.integers(G, 41)))])[:G]                    # distinct; repeats of slot keys among them
        gslot, hit = plan(skey, sstate, sused, gkey)
        where = {int(skey[s]): int(s) for s in full}
        # every hit keeps its slot, and nothing else counts as a hit
        for g in range(G):
            assert hit[g] == (int(gkey[g]) in where), (g, gkey, skey, sstate)
            if hit[g]:
                assert gslot[g] == where[int(gkey[g])]
        # no two groups share a slot; a miss never takes a slot that was hit in this call
        assert all(0 <= s < SLOTS for s in gslot) and len(set(int(s) for s in gslot)) == G
        hit_slots = {int(gslot[g]) for g in range(G) if hit[g]}
        miss_slots = [int(gslot[g]) for g in range(G) if not hit[g]]
        assert not hit_slots & set(miss_slots)
        # empty slots go before used ones; among the used ones the oldest goes first
        left = [s for s in range(SLOTS) if s not in hit_slots and s not in miss_slots]
        used_taken = [s for s in miss_slots if sstate[s] == 1]
        if used_taken:
            assert not any(sstate[s] == 0 for s in left), (gslot, sstate)
            assert all(sused[u] >= max(sused[s] for s in used_taken) for u in left if sstate[u] == 1), (gslot, sused, sstate)
            # in the order of the groups: each miss took the oldest used slot that was left for it
            assert [sused[s] for s in used_taken] == sorted(sused[s] for s in used_taken)
            seen_evict += 1
        seen_hit += any(hit)
        seen_mixed += any(hit) and bool(used_taken)
    assert seen_hit > 1000 and seen_evict > 1000 and seen_mixed > 300, (seen_hit, seen_evict, seen_mixed)
