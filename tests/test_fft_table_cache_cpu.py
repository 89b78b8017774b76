"""The policy of the per-size FFT table cache (bellman_amd/csrc/fft_tables_plan.hpp) without a GPU: the library's own rules
(bh_test_fft_table_policy, host only) drive the simulated cache of tests/models/fft_table_model.py, every decision is compared
with the model's restatement, and after every step the properties the cache promises are checked - including the branches
behind a failed allocation, which no GPU test may provoke.

What "within the budget" means here, as the cache has always behaved: the budget gates the ONE-LEVEL tables (n entries each).
The two-level tables (about 2^(log_n/2) entries) and the 48-byte 1/n entry of a size are built whatever the budget is - a
budget of 0 still transforms - so the check is made where a call built one-level tables: the cache's bytes before the call
plus the new tables fit the budget, or the call is the one documented exception, a size that already ran on one-level tables
and was alone in the cache completing its own set after the budget had been lowered under it."""

import ctypes
import itertools
import random

import numpy as np
import pytest

from tests.models import fft_table_model as fm

ZINV = (0, False, False, False)      # cached_zinv: a call that needs no table


def _requests(log_n):
    return [fm.request(log_n, mode) for mode in range(4)] + [ZINV]


class HookRules:
    """the library's rules; every answer is compared with the model's before it is used"""

    def __init__(self):
        from bellman_amd import _lib
        self.lib = _lib.load()
        self.compared = [0, 0, 0]

    def _call(self, rule, words):
        a = np.array([int(w) for w in words], dtype=np.uint64)
        out = np.zeros(4, dtype=np.uint64)
        rc = self.lib.bh_test_fft_table_policy(rule, a.ctypes.data_as(ctypes.c_void_p), len(a), out.ctypes.data_as(ctypes.c_void_p))
        assert rc == 0, (rule, words, rc)
        self.compared[rule] += 1
        return [int(x) for x in out]

    def decide(self, *args):
        got = tuple(self._call(0, args))
        assert got == fm.Rules.decide(*args), (args, got)
        return got

    def build_failed(self, *args):
        got = self._call(1, args)[0]
        assert got == fm.Rules.build_failed(*args), (args, got)
        return got

    def evict_victim(self, entries, keep_log_n, cache_bytes, need, budget):
        got = self._call(2, [keep_log_n, cache_bytes, need, budget] + [w for e in entries for w in e])[0]
        got = -1 if got == (1 << 64) - 1 else got
        assert got == fm.Rules.evict_victim(entries, keep_log_n, cache_bytes, need, budget), (entries, keep_log_n, cache_bytes, need, got)
        return got


@pytest.fixture(scope="module")
def rules():
    return HookRules()


def _size_bytes(log_n, s):
    """what a size's holdings weigh, counted table by table"""
    per_role = (lambda role: fm.one_level_role_bytes(role, log_n)) if s.kind == fm.ONE_LEVEL else (lambda role: fm.two_level_role_bytes(log_n))
    return fm.MINV_BYTES + sum(per_role(role) for role in s.tables)


def _step(cache, log_n, req, fail_at=()):
    """one call with the invariants checked around it; returns the call's record"""
    before = {k: s.snapshot() for k, s in cache.sizes.items()}
    total, tick = cache.total, cache.tick
    had = cache.held(log_n)
    had_kind, had_bytes = had.kind, had.bytes
    rec = cache.call(log_n, req, fail_at)
    where = (log_n, req, sorted(fail_at), cache.budget, rec)
    # a size never holds both kinds, and has a kind exactly when it holds a table
    for k, s in cache.sizes.items():
        assert set(s.tables.values()) == ({s.kind} if s.kind else set()), where
        assert s.bytes == _size_bytes(k, s) and s.bytes, where
        if s.kind == fm.ONE_LEVEL:
            assert cache.one_level_enabled and 12 <= k <= 24, where
    assert cache.total == sum(s.bytes for s in cache.sizes.values()) == rec["total"], where
    for k in rec["evicted"]:
        assert k != log_n and k in before and k not in cache.sizes, where
    for k, snap in before.items():
        if k != log_n and k not in rec["evicted"]:
            assert cache.sizes[k].snapshot() == snap, where      # other sizes: dropped or untouched
    if rec["ok"]:
        s = cache.sizes[log_n]
        assert not fm.roles_needed(*req) & ~s.roles, where        # every role the request needs, in the size's kind
        assert s.last_use == cache.tick == tick + 1, where
        if rec["kind"] == fm.ONE_LEVEL:
            # what the cache held when the call decided (after its evictions) plus the new one-level tables
            fits = cache.total - (0 if had_bytes else fm.MINV_BYTES) <= cache.budget
            assert fits != rec["over_budget"], where
            if not fits:
                assert had_kind == fm.ONE_LEVEL and list(cache.sizes) == [log_n], where
                assert s.bytes <= fm.one_level_set_bytes(log_n) + fm.MINV_BYTES, where
        else:
            assert not rec["over_budget"], where
    else:
        # a failed call leaves its size as it was (and, where it evicted nothing, the whole cache)
        assert (cache.sizes[log_n].snapshot() if log_n in cache.sizes else None) == before.get(log_n), where
        assert cache.tick == tick and (rec["evicted"] or cache.total == total), where
        assert fail_at, where                                      # only an allocation failure fails a call
    return rec


def _budgets(sizes):
    """no budget, every complete set on its edge, everything at once"""
    sets = [fm.one_level_set_bytes(k) for k in sizes]
    return sorted({0, sum(sets) + (1 << 20)} | {s + d for s in sets for d in (-1, 0)})


def test_every_short_sequence_over_two_sizes(rules):
    """every sequence of three calls over 2^12 and 2^13 (the four transforms and a table-less call each), under every pair
    of budgets - the budget changes before the last call -, the last call also with an allocation failure at each of its
    build positions (and at all of them)"""
    sizes = (12, 13)
    steps = [(k, req) for k in sizes for req in _requests(k)]
    budgets = _budgets(sizes)
    seen = set()
    for b1 in budgets:
        for first in itertools.product(steps, repeat=2):
            start = fm.Cache(b1, True, rules)
            for log_n, req in first:
                _step(start, log_n, req)
            for (log_n, req), b2 in itertools.product(steps, budgets):
                for fail_at in [()] + ([(i,) for i in range(4)] + [tuple(range(16))] if b1 == b2 else []):
                    cache = start.copy()
                    cache.budget = b2
                    rec = _step(cache, log_n, req, fail_at)
                    seen |= {name for name in ("evicted", "forced_two_level", "over_budget", "fell_back") if rec[name]}
                    if not rec["ok"]:
                        seen.add("failed")
    # (a rebuild after an eviction takes more than three calls: the sampled sequences below reach it)
    assert seen == {"evicted", "forced_two_level", "over_budget", "fell_back", "failed"}, seen
    assert all(n > 1000 for n in rules.compared[:2]) and rules.compared[2] > 100, rules.compared


@pytest.mark.parametrize("one_level_enabled", [True, False])
def test_sampled_sequences_over_every_size(rules, one_level_enabled):
    """2^8 ... 2^26 points, all four modes and table-less calls, budgets from 0 to "everything fits" lowered and raised on
    the way, the one-level switch on and off, allocation failures at a build position of every kind"""
    rnd = random.Random(20240 + one_level_enabled)
    sizes = list(range(8, 27))
    everything = sum(fm.one_level_set_bytes(k) for k in range(12, 25)) + (1 << 30)
    seen, outcomes = set(), set()
    for _ in range(150):
        pool = rnd.sample(sizes, rnd.randint(2, 6))
        budgets = [0, everything] + [fm.one_level_set_bytes(k) + rnd.choice((-1, 0, 4096)) for k in pool if 12 <= k <= 24]
        budgets += [sum(rnd.sample(budgets, 2))]
        cache = fm.Cache(rnd.choice(budgets), one_level_enabled, rules)
        for _ in range(40):
            if rnd.random() < 0.15:
                cache.budget = rnd.choice(budgets)
            log_n = rnd.choice(pool)
            fail_at = ()
            if rnd.random() < 0.2:
                fail_at = rnd.choice([(rnd.randrange(5),), (0, 1, 2), tuple(range(16))])
            rec = _step(cache, log_n, rnd.choice(_requests(log_n)), fail_at)
            seen |= {name for name in ("evicted", "rebuilt", "forced_two_level", "over_budget", "fell_back") if rec[name]}
            outcomes.add(rec["ok"])
            assert one_level_enabled or rec["kind"] in (None, fm.TWO_LEVEL)
    assert outcomes == {True, False}
    if one_level_enabled:
        assert seen == {"evicted", "rebuilt", "forced_two_level", "over_budget", "fell_back"}, seen
    else:
        assert not seen, seen       # two-level tables only: nothing is gated, evicted or redone


def test_byte_counts_and_refusals(rules):
    """the sizes of the issue's table (a one-level table and a complete set at 2^12 ... 2^15), a two-level pair, and what the
    hook refuses"""
    assert [fm.one_level_table_bytes(k) >> 10 for k in (12, 13, 14, 15)] == [128, 256, 512, 1024]
    assert [fm.one_level_set_bytes(k) >> 10 for k in (12, 13, 14, 15)] == [512, 1024, 2048, 4096]
    assert fm.one_level_set_bytes(23) == 6 * (32 << 23)                    # three passes: two tables per direction
    assert fm.two_level_role_bytes(13) == (128 + 64) * 48 and fm.two_level_role_bytes(16) == 512 * 48
    lib = rules.lib
    out = np.zeros(4, dtype=np.uint64)
    o = out.ctypes.data_as(ctypes.c_void_p)

    def call(rule, words):
        a = np.array(words, dtype=np.uint64)
        return lib.bh_test_fft_table_policy(rule, a.ctypes.data_as(ctypes.c_void_p), len(a), o)

    assert call(0, [0, 0, 0, 12, 0, 1, 0, 0, 0, 1 << 30, 1]) == 0 and [int(x) for x in out] == [0, 1, 1, 48 + (128 << 10)]
    assert call(0, [0, 0, 0, 32, 0, 1, 0, 0, 0, 1 << 30, 1]) < 0          # no such domain
    assert call(0, [0, 0, 0, 12, 0, 1, 0, 0, 0, 1 << 30]) < 0             # a word short
    assert call(1, [0, 0, 0]) < 0 and call(2, [12, 0, 0, 0, 13, 48]) < 0 and call(3, [0]) < 0
    assert call(2, [12, 0, 0, 0]) == 0 and int(out[0]) == (1 << 64) - 1    # an empty cache: nothing to drop
