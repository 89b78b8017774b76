"""The per-size FFT table cache on the GPU (run with `pytest -m gpu` on a MI355X), through the public API only
(Worker.set_limits, Worker.info, EvaluationDomain): its policy at the smallest sizes that have one-level tables, byte for
byte against the simulated cache of tests/models/fft_table_model.py (whose rules tests/test_fft_table_cache_cpu.py compares
with the library's own, csrc/fft_tables_plan.hpp), and the two tests at 2^20 ... 2^24 points that guard the budget and the
lock protocol of an eviction between host threads.  Integer work: every limb equal, no tolerances."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_gpu_groth16 import worker  # noqa: E402,F401


def test_fft_table_policy_at_the_smallest_one_level_sizes():
    """A budget of 2.5 MiB: the complete one-level sets of 2^12 and 2^13 (512 KiB, 1 MiB) fit together, 2^14's (2 MiB) fits
    alone but not beside them, 2^15's (4 MiB) does not fit at all.  fft, ifft, coset_fft and icoset_fft over 12, 13, 14, 12,
    15, 14; then 2^13 again, the budget lowered below what is held and 2^13's set finished; then no budget at all, a fresh
    size and one whose tables were dropped.  After every call bh_ctx_info's fft_table_bytes is what the simulated cache
    predicts, to the byte, and the data is the restated best_fft's (src/domain.rs:81-125), bit for bit; the model's trace
    must show an eviction, a rebuild after one, a size the budget forces onto two-level tables, and a set completed over a
    lowered budget - so the test cannot pass on a sequence that stopped reaching them."""
    import bellman_amd
    from oracle import cref
    from tests.models import fft_table_model as fm

    budget = 5 << 19
    sets = {k: fm.one_level_set_bytes(k) + fm.MINV_BYTES for k in (12, 13, 14, 15)}
    assert sets[12] + sets[13] <= budget and sets[14] <= budget < sets[14] + min(sets[12], sets[13]) and sets[15] > budget
    cache = fm.Cache(budget)
    data, want, trace = {}, {}, []
    w = bellman_amd.Worker(0)
    try:
        w.set_limits(fft_table_budget_bytes=budget)
        assert w.info()["fft_table_budget"] == budget and w.info()["fft_table_bytes"] == 0

        def transform(log_n, mode):
            if log_n not in data:
                data[log_n] = cref.random_fr(1 << log_n, 5150 + log_n)
            if (log_n, mode) not in want:
                want[log_n, mode] = cref.fft(data[log_n], mode)
            d = bellman_amd.EvaluationDomain.from_coeffs(w, data[log_n])
            [d.fft, d.ifft, d.coset_fft, d.icoset_fft][mode]()
            rec = cache.transform(log_n, mode)
            trace.append(rec)
            assert rec["ok"] and w.info()["fft_table_bytes"] == rec["total"], (log_n, mode, w.info()["fft_table_bytes"], rec)
            assert np.array_equal(d.into_coeffs(), want[log_n, mode]), (log_n, mode)
            return rec

        for log_n in (12, 13, 14, 12, 15, 14):
            for mode in range(4):
                transform(log_n, mode)
        assert any(r["evicted"] for r in trace) and any(r["rebuilt"] and r["kind"] == fm.ONE_LEVEL for r in trace)
        assert any(r["forced_two_level"] for r in trace) and all(r["kind"] == fm.TWO_LEVEL for r in trace if r["log_n"] == 15)
        assert all(r["total"] <= budget for r in trace)
        # the budget lowered under a size that runs on one-level tables: it completes its set, alone in the cache
        transform(13, 0)
        lowered = fm.one_level_table_bytes(13)   # (less than 2^13 itself holds by now)
        w.set_limits(fft_table_budget_bytes=lowered)
        cache.budget = lowered
        over = [transform(13, mode) for mode in (1, 2, 3)]
        assert all(r["over_budget"] and r["kind"] == fm.ONE_LEVEL for r in over) and over[0]["evicted"]
        assert list(cache.sizes) == [13] and cache.total == sets[13] > lowered
        # no budget at all: two-level tables, at a fresh size and at one whose tables (and kind) an eviction dropped
        w.set_limits(fft_table_budget_bytes=0)
        cache.budget = 0
        for log_n in (11, 12):
            for mode in range(4):
                assert transform(log_n, mode)["kind"] in (None, fm.TWO_LEVEL)
        assert cache.sizes[12].kind == fm.TWO_LEVEL and cache.sizes[13].kind == fm.ONE_LEVEL
    finally:
        w.close()


def test_fft_table_cache_stays_within_its_budget(worker):
    """[r5] The per-size FFT tables are a cache with a budget (bh_ctx_set_limits' fft_table_budget_bytes, reported by
    bh_ctx_info): under 768 MiB the transforms of 2^20 ... 2^24 points - whose one-level tables would add up to several
    GiB - stay exact (fft against the restated best_fft up to 2^22, ifft . fft and icoset_fft . coset_fft back to the data at
    every size: src/domain.rs:81-125, :427-463; both table kinds limb for limb: tests/test_gpu_fft_extremes.py), `fft_table_bytes` never
    exceeds the budget, sizes whose complete set does not fit run on the two-level tables, and coming back to an evicted
    size rebuilds its tables."""
    import bellman_amd
    from oracle import cref

    budget = 768 << 20   # 2^20 + 2^21 + 2^22 need 128 + 256 + 512 MiB of one-level tables: the third size evicts the first
    w = bellman_amd.Worker(0)
    try:
        w.set_limits(fft_table_budget_bytes=budget)
        assert w.info()["fft_table_budget"] == budget and w.info()["fft_table_bytes"] == 0
        seen, checked = [], set()
        for log_n in (20, 21, 22, 23, 24, 20, 22):
            data = cref.random_fr(1 << log_n, 7700 + log_n)
            d = bellman_amd.EvaluationDomain.from_coeffs(w, data)
            for step, mode in enumerate((0, 1, 2, 3)):   # fft, ifft (back to the data), coset_fft, icoset_fft (back again)
                [d.fft, d.ifft, d.coset_fft, d.icoset_fft][mode]()
                held = w.info()["fft_table_bytes"]
                assert held <= budget, (log_n, mode, held)
                seen.append(held)
                if mode == 0 and log_n <= 22 and log_n not in checked:   # (8 threads: the oracle's split costs m * P products)
                    assert np.array_equal(d.as_ref(), cref.fft(data, 0, threads=8)), log_n
                    checked.add(log_n)
                if mode in (1, 3):
                    assert np.array_equal(d.as_ref(), data), (log_n, mode)
            d.into_coeffs()
        assert max(seen) > (64 << 20)    # one-level tables were in use (2^20: 32 MiB each) ...
        assert any(b < a for a, b in zip(seen, seen[1:]))   # ... and the least recently used size made room at least once
        w.set_limits(fft_table_budget_bytes=0)   # ... and with no budget at all every size runs on two-level tables
        data = cref.random_fr(1 << 16, 7777)
        d = bellman_amd.EvaluationDomain.from_coeffs(w, data)
        d.icoset_fft()
        assert np.array_equal(d.into_coeffs(), cref.fft(data, 3, threads=8))
    finally:
        w.close()


def test_fft_cache_eviction_between_two_host_threads_always_completes():
    """[r6, ADVICE r5] Two host threads transform sizes whose one-level table sets do NOT fit the cache's budget together
    (2^21: 4 x 64 MiB, 2^22: 4 x 128 MiB under 640 MiB), so each call of one thread may have to evict the other's tables.
    Round 5 retried that four times under the shared use lock and returned BH_ERR_HIP when the threads kept evicting each
    other; the eviction path now holds the use lock exclusively through the rebuild.  Every call must succeed, every round
    trip (ifft . fft, icoset_fft . coset_fft: src/domain.rs:81-125) must give the data back, the budget must hold."""
    import threading

    import bellman_amd
    from oracle import cref

    budget = 640 << 20
    w = bellman_amd.Worker(0)
    errors, held = [], []
    try:
        w.set_limits(fft_table_budget_bytes=budget)

        def run(log_n, rounds):
            try:
                data = cref.random_fr(1 << log_n, 4400 + log_n)
                d = bellman_amd.EvaluationDomain.from_coeffs(w, data)
                for i in range(rounds):
                    d.fft()
                    d.ifft()
                    d.coset_fft()
                    d.icoset_fft()
                    held.append(w.info()["fft_table_bytes"])
                    if i % 8 == 7 and not np.array_equal(d.as_ref(), data):
                        errors.append("round trip at 2^%d, round %d" % (log_n, i))
                if not np.array_equal(d.into_coeffs(), data):
                    errors.append("final round trip at 2^%d" % log_n)
            except Exception as e:   # a spurious BH_ERR_HIP surfaces here
                errors.append("2^%d: %r" % (log_n, e))

        threads = [threading.Thread(target=run, args=(21, 40)), threading.Thread(target=run, args=(22, 40))]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors[:4]
        assert max(held) <= budget
    finally:
        w.close()
