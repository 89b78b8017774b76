"""Executable model of the per-size FFT table cache of bellman_amd/csrc/fft.hip: the three rules of its policy
(csrc/fft_tables_plan.hpp: what a call builds, what follows a failed one-level build, which size an eviction drops) restated,
and a simulation of the whole cache around them - a map of sizes, the total bytes, a tick counter - that walks the steps of
get_tables / acquire_tables / fft_evict_locked without a GPU.

The byte count is the library's (bh_ctx_info's fft_table_bytes): every cached size holds a 48-byte 1/n entry, the shared
master tables are left out, a two-level role is a lo / hi pair of (2^lb + 2^(log_n - lb)) * 48 bytes with lb = ceil(log_n / 2),
a one-level table is 32 << log_n bytes and a twiddle role has one per non-last pass.

`Cache` takes the rules as an object, so a test can run the same simulation on the library's own rules
(bh_test_fft_table_policy) and compare every decision with the ones here."""

from tests.models.ntt_model import plan_passes

NONE, ONE_LEVEL, TWO_LEVEL = 0, 1, 2                    # FftTableKind
TW_FWD, TW_INV, COSET, ICOSET = 0, 1, 2, 3              # FftTableRole
ROLES = 4
FALL_BACK, EVICT_ALL_AND_RETRY, FAIL = 0, 1, 2          # FftBuildFailure
EVICT_ALL = (1 << 64) - 1
MINV_BYTES = 48
FFT, IFFT, COSET_FFT, ICOSET_FFT = 0, 1, 2, 3           # BH_FFT ... BH_ICOSET_FFT


def passes(log_n):
    return len(plan_passes(log_n))


def one_level_table_bytes(log_n):
    return 32 << log_n


def one_level_role_bytes(role, log_n):
    return (passes(log_n) - 1 if role in (TW_FWD, TW_INV) else 1) * one_level_table_bytes(log_n)


def one_level_set_bytes(log_n):
    return sum(one_level_role_bytes(role, log_n) for role in range(ROLES))


def two_level_role_bytes(log_n):
    lb = (log_n + 1) // 2
    return ((1 << lb) + (1 << (log_n - lb))) * 48


def role_list(mask):
    return [role for role in range(ROLES) if mask >> role & 1]


def build_bytes(held_bytes, kind, roles, log_n):
    per_role = (lambda role: one_level_role_bytes(role, log_n)) if kind == ONE_LEVEL else (lambda role: two_level_role_bytes(log_n))
    return (0 if held_bytes else MINV_BYTES) + sum(per_role(role) for role in role_list(roles))


def request(log_n, mode):
    """(dir, need_tw, need_coset, need_icoset) of a transform, as ntt_run asks for its tables"""
    return int(mode in (IFFT, ICOSET_FFT)), passes(log_n) > 1, mode == COSET_FFT, mode == ICOSET_FFT


def roles_needed(dir, need_tw, need_coset, need_icoset):
    return (1 << (TW_FWD + dir) if need_tw else 0) | (1 << COSET if need_coset else 0) | (1 << ICOSET if need_icoset else 0)


class Rules:
    """the policy, restated: every method returns plain integers, as the library's hook does"""

    @staticmethod
    def decide(kind, roles, held_bytes, log_n, dir, need_tw, need_coset, need_icoset, cache_bytes, budget, one_level_enabled):
        """-> (evict_need, kind, roles, bytes)"""
        build_kind = kind
        if build_kind == NONE:   # a size that holds tables keeps their kind
            fits = one_level_enabled and 12 <= log_n <= 24 and one_level_set_bytes(log_n) <= budget
            build_kind = ONE_LEVEL if fits else TWO_LEVEL
        build = roles_needed(dir, need_tw, need_coset, need_icoset) & ~roles
        if build_kind == ONE_LEVEL:
            need = sum(one_level_role_bytes(role, log_n) for role in role_list(build))
            if need and cache_bytes + need > budget:
                if cache_bytes > held_bytes:        # other sizes to drop
                    return need, build_kind, build, 0
                if kind != ONE_LEVEL:               # the budget was lowered under this call
                    build_kind = TWO_LEVEL
                # (a size that already runs on one-level tables completes its set over the budget)
        return 0, build_kind, build, build_bytes(held_bytes, build_kind, build, log_n)

    @staticmethod
    def build_failed(kind, roles, held_bytes, other_bytes):
        if other_bytes:
            return EVICT_ALL_AND_RETRY
        return FAIL if kind == ONE_LEVEL else FALL_BACK

    @staticmethod
    def evict_victim(entries, keep_log_n, cache_bytes, need, budget):
        """entries: [(log_n, bytes, last_use)] -> index of the next victim, -1: done"""
        if need != EVICT_ALL and cache_bytes + need <= budget:
            return -1
        victim = -1
        for i, (log_n, held, last_use) in enumerate(entries):
            if log_n != keep_log_n and held and (victim < 0 or last_use < entries[victim][2]):
                victim = i
        return victim


class Size:
    def __init__(self):
        self.kind, self.bytes, self.last_use = NONE, 0, 0
        self.tables = {}          # role -> the kind its tables were built in

    @property
    def roles(self):
        return sum(1 << role for role, kind in self.tables.items() if kind == self.kind)

    def snapshot(self):
        return (self.kind, self.bytes, self.last_use, tuple(sorted(self.tables.items())))


class Cache:
    """The table cache of one context.  `call` is acquire_tables; its result is a record of what happened:
      ok            the call succeeded
      evicted       the sizes dropped on the way, in order
      kind, built   the kind and the roles whose tables the call built (kind None: it built none)
      rebuilt       it built tables for a size that an eviction had dropped before
      forced_two_level  it built two-level tables, because of the budget, at a size the one-level tables exist for
      over_budget   it completed a one-level set beyond the budget (which had been lowered under that size)
      fell_back     a failed one-level build was redone two-level
      total         the cache's bytes afterwards
    fail_at: the ordinals of the call's device allocations that fail (0 is its first allocation; the master tables, which
    are not the cache's, are not counted)."""

    def __init__(self, budget, one_level_enabled=True, rules=Rules):
        self.budget, self.one_level_enabled, self.rules = budget, one_level_enabled, rules
        self.sizes, self.total, self.tick = {}, 0, 0
        self.dropped = set()

    def copy(self):
        c = Cache(self.budget, self.one_level_enabled, self.rules)
        c.total, c.tick, c.dropped = self.total, self.tick, set(self.dropped)
        for log_n, s in self.sizes.items():
            t = c.sizes[log_n] = Size()
            t.kind, t.bytes, t.last_use, t.tables = s.kind, s.bytes, s.last_use, dict(s.tables)
        return c

    def held(self, log_n):
        return self.sizes.get(log_n) or Size()

    def _evict(self, keep_log_n, need, rec):
        entries = [(log_n, s.bytes, s.last_use) for log_n, s in sorted(self.sizes.items())]
        while True:
            v = self.rules.evict_victim(entries, keep_log_n, self.total, need, self.budget)
            if v < 0:
                return
            log_n = entries[v][0]
            assert log_n != keep_log_n and entries[v][1], "an eviction never drops the caller's size or an empty one"
            self.total -= self.sizes.pop(log_n).bytes
            self.dropped.add(log_n)
            rec["evicted"].append(log_n)
            entries[v] = (log_n, 0, entries[v][2])

    def _get_tables(self, log_n, req, rec, alloc):
        """-> "ok", "fail" or ("evict", need)"""
        h = self.held(log_n)
        others = self.total - h.bytes
        need, kind, build, cost = self.rules.decide(h.kind, h.roles, h.bytes, log_n, *req, self.total, self.budget, self.one_level_enabled)
        if need:
            return "evict", need
        if not h.bytes and not alloc():          # the 1/n entry
            return "fail"

        def build_tables(kind):
            per_role = 2 if kind == TWO_LEVEL else None
            for role in role_list(build):
                for _ in range(per_role or one_level_role_bytes(role, log_n) // one_level_table_bytes(log_n)):
                    if not alloc():
                        return False
            return True

        ok = build_tables(kind)
        if not ok and kind == ONE_LEVEL:
            outcome = self.rules.build_failed(h.kind, h.roles, h.bytes, others)
            if outcome == EVICT_ALL_AND_RETRY:
                return "evict", EVICT_ALL
            if outcome == FAIL:
                return "fail"
            assert outcome == FALL_BACK
            kind, cost = TWO_LEVEL, build_bytes(h.bytes, TWO_LEVEL, build, log_n)
            rec["fell_back"] = True
            ok = build_tables(kind)
        if not ok:
            return "fail"
        in_window = self.one_level_enabled and 12 <= log_n <= 24
        if build:
            rec["kind"], rec["built"] = kind, build
            rec["rebuilt"] = log_n in self.dropped
            rec["forced_two_level"] = kind == TWO_LEVEL and in_window and not rec["fell_back"] and h.kind == NONE
            rec["over_budget"] = kind == ONE_LEVEL and self.total + cost - (0 if h.bytes else MINV_BYTES) > self.budget
            h.kind = kind
            for role in role_list(build):
                h.tables[role] = kind
        h.bytes += cost
        self.tick += 1
        h.last_use = self.tick
        self.total += cost
        self.sizes[log_n] = h
        return "ok"

    def call(self, log_n, req, fail_at=()):
        rec = dict(log_n=log_n, req=req, ok=False, evicted=[], kind=None, built=0, rebuilt=False, forced_two_level=False, over_budget=False,
                   fell_back=False)
        count = [0]

        def alloc():
            count[0] += 1
            return count[0] - 1 not in fail_at

        rc = self._get_tables(log_n, req, rec, alloc)
        for attempt in range(2):      # (second round: everything else goes)
            if rc in ("ok", "fail"):
                break
            self._evict(log_n, EVICT_ALL if attempt else rc[1], rec)
            rc = self._get_tables(log_n, req, rec, alloc)
        # the termination argument of acquire_tables: with every other size gone no eviction is asked for again
        assert rc in ("ok", "fail"), "an eviction was asked for after every other size had gone"
        rec["ok"] = rc == "ok"
        rec["total"] = self.total
        return rec

    def transform(self, log_n, mode, fail_at=()):
        return self.call(log_n, request(log_n, mode), fail_at)
