"""The MSM pipeline over the context's three streams (front / accumulation / tail): jobs of the general
kernels in every slot at once, of mixed kinds, collected out of order, with timing, with a one-launch job, batches, an error,
host-pointer calls from four threads and a new SRS between them.  An SRS of 16 385 points and polynomials of 8 193 to 16 385
coefficients: more than 65 536 bucket references per job, so every job takes the sort / accumulation / tail hand-overs and not
k_small_msm, and the oracle's bucket method answers in milliseconds.  Every expected point comes from the oracle
(oracle_ctypes), never from another call of the library; integer work, compared bit for bit as compressed encodings."""
import ctypes as C
import math
import threading

import numpy as np
import pytest

import kzg_poly_commit_exploration_amd as K

pytestmark = pytest.mark.gpu

SRS_N = 16385
MIN_N = 8193
SECRET = bytes(range(7, 39))


def _poly(seed, n):
    """n coefficients as blst_fr rows: any value below 2^254 < r is the Montgomery image of some scalar"""
    a = np.random.default_rng(seed).integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    a[:, 3] &= np.uint64((1 << 62) - 1)
    return np.ascontiguousarray(a)


def _point(seed):
    z = np.random.default_rng(1000003 + seed).integers(0, 1 << 62, size=4, dtype=np.uint64)
    return np.ascontiguousarray(z)


class _Expected:
    """the oracle's answers, each computed once and handed out to every test that needs it"""

    def __init__(self, oracle):
        self.oracle = oracle
        self.srs = oracle.srs_g1(SRS_N, SECRET)
        self.commits, self.proofs = {}, {}

    def commit(self, seed, n, srs_n=SRS_N):
        key = (seed, n, srs_n)
        if key not in self.commits:
            rc, p = self.oracle.commit_pippenger(_poly(seed, n), self.srs[:srs_n])
            assert rc == 0
            self.commits[key] = self.oracle.p1_compress(p)
        return self.commits[key]

    def opening(self, seed, n, srs_n=SRS_N):
        """(z, y, proof) of polynomial `seed` at the point of the same seed"""
        key = (seed, n, srs_n)
        if key not in self.proofs:
            c, z = _poly(seed, n), _point(seed)
            y = self.oracle.poly_evaluate(c, z)
            rc, q = self.oracle.quotient(c, z, y)
            assert rc == 0 and len(q) == n - 1
            rc, p = self.oracle.commit_pippenger(q, self.srs[:srs_n])
            assert rc == 0
            self.proofs[key] = (K.Scalar.from_limbs(z), K.Scalar.from_limbs(y), self.oracle.p1_compress(p))
        return self.proofs[key]


@pytest.fixture(scope="module")
def expected(oracle):
    return _Expected(oracle)


@pytest.fixture(scope="module")
def eng():
    e = K.Engine(0)
    e.srs_generate(SECRET, SRS_N)
    yield e
    e.close()


class _Resident:
    """polynomials in device memory for the length of a test"""

    def __init__(self, eng):
        self.eng, self.ptrs = eng, []

    def put(self, array):
        a = np.ascontiguousarray(array, dtype=np.uint64)
        p = self.eng.dev_alloc(a.nbytes)
        self.ptrs.append(p)
        self.eng.dev_upload(p, a)
        return p

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.eng.dev_free(p)


def _length(job):
    """distinct lengths from MIN_N up to SRS_N, odd and even, first and last at the two ends"""
    return min(SRS_N, MIN_N + 547 * job) if job else SRS_N


def _rounds(eng, expected, rounds=3, timing=False):
    """`rounds` rounds over all slots, commitments and openings alternating, no wait inside a round, collected in reverse
    slot order; returns times(slot) of every job with its kind"""
    slots = eng.num_slots()
    jobs = [(r * slots + s, s, (r * slots + s) % 2 == 1) for r in range(rounds) for s in range(slots)]
    assert len({_length(j) for j, _, _ in jobs}) == len(jobs)
    seen = []
    with _Resident(eng) as dev:
        ptrs = {j: dev.put(_poly(j, _length(j))) for j, _, _ in jobs}
        wanted = {j: (expected.opening(j, _length(j)) if is_open else expected.commit(j, _length(j))) for j, _, is_open in jobs}
        for r in range(rounds):
            this = [x for x in jobs if x[0] // slots == r]
            for j, s, is_open in this:
                if is_open:
                    z, y, _ = wanted[j]
                    eng.open_submit(s, ptrs[j], _length(j), z, y)
                else:
                    eng.commit_submit(s, ptrs[j], _length(j))
            for j, s, is_open in reversed(this):
                got = eng.wait(s).compress()
                assert got == (wanted[j][2] if is_open else wanted[j]), (r, s, "open" if is_open else "commit")
                if timing:
                    seen.append((is_open, eng.times(s)))
    return seen


def test_every_slot_busy_mixed_kinds_collected_out_of_order(eng, expected):
    """A `done` event left on the wrong stream, or a slot reused before its tail ended, returns the previous round's point."""
    _rounds(eng, expected)


def test_every_slot_busy_with_timing(eng, expected):
    eng.set_timing(True)
    try:
        seen = _rounds(eng, expected, timing=True)
    finally:
        eng.set_timing(False)
    assert len(seen) == 3 * eng.num_slots()
    for is_open, t in seen:
        for name, v in t.items():
            assert math.isfinite(v) and v >= 0, (name, v, t)
        assert t["references"] > 65536, t  # the general kernels, not the one-launch path
        assert t["accumulate_ms"] > 0 and t["accumulate_events_ms"] > 0, t
        if is_open:
            assert t["quotient_ms"] > 0, t


def test_small_job_between_two_general_ones(eng, expected, oracle):
    small = oracle.bench_coefficients(101)
    rc, want_small = oracle.commit_pippenger(small, expected.srs[:101])
    assert rc == 0
    with _Resident(eng) as dev:
        a, b = dev.put(_poly(0, _length(0))), dev.put(_poly(2, _length(2)))
        s = dev.put(small)
        eng.commit_submit(0, a, _length(0))
        eng.commit_submit(1, s, 101)
        eng.commit_submit(2, b, _length(2))
        assert eng.wait(0).compress() == expected.commit(0, _length(0))
        assert eng.wait(1).compress() == oracle.p1_compress(want_small)
        assert eng.wait(2).compress() == expected.commit(2, _length(2))


def test_batches_on_two_slots_back_to_back(eng, expected):
    n = _length(1)
    seeds = [21, 22, 23, 24]
    polys = [_poly(sd, n) for sd in seeds]
    try:
        assert eng.set_max_batch(2) == 2
        with _Resident(eng) as dev:
            d0, d1 = dev.put(np.concatenate(polys[:2])), dev.put(np.concatenate(polys[2:]))
            eng.commit_batch_submit(0, d0, n, 2)
            eng.commit_batch_submit(1, d1, n, 2)
            got = eng.wait_batch(0, 2) + eng.wait_batch(1, 2)
            for g, sd in zip(got, seeds):
                assert g.compress() == expected.commit(sd, n), sd
            opens = [expected.opening(sd, n) for sd in seeds]
            zl = np.ascontiguousarray(np.stack([o[0].limbs() for o in opens]))
            yl = np.ascontiguousarray(np.stack([o[1].limbs() for o in opens]))
            for slot, d in ((0, d0), (1, d1)):
                K._check(eng._lib.kzg_open_batch_submit(eng._h, slot, C.c_void_p(d), n, 2, n, K._ptr(zl[2 * slot:]), K._ptr(yl[2 * slot:])),
                         eng._h)
            for slot in (0, 1):
                out = np.zeros((2, 18), dtype=np.uint64)
                st = np.zeros(2, dtype=np.int32)
                K._check(eng._lib.kzg_wait_open_batch(eng._h, slot, K._ptr(out), K._ptr(st), 2), eng._h)
                for i in range(2):
                    assert st[i] == K.KZG_OK
                    assert K.G1Point(out[i]).compress() == opens[2 * slot + i][2], (slot, i)
    finally:
        assert eng.set_max_batch(1) == 1  # the workspaces are reallocated: everything in flight is drained first
    with _Resident(eng) as dev:
        eng.commit_submit(3, dev.put(_poly(4, _length(4))), _length(4))
        assert eng.wait(3).compress() == expected.commit(4, _length(4))


def test_error_between_good_jobs(eng, expected):
    n_bad = SRS_N + 3
    bad = _poly(77, n_bad)  # every coefficient is odd, so the ones beyond the SRS are non-zero
    with _Resident(eng) as dev:
        a, b, c = dev.put(_poly(6, _length(6))), dev.put(bad), dev.put(_poly(8, _length(8)))
        eng.commit_submit(0, a, _length(6))
        eng.commit_submit(1, b, n_bad)
        eng.commit_submit(2, c, _length(8))
        assert eng.wait(2).compress() == expected.commit(8, _length(8))
        with pytest.raises(K.KzgError) as ei:
            eng.wait(1)
        assert ei.value.status == K.KZG_ERR_DEGREE_TOO_HIGH
        assert eng.wait(0).compress() == expected.commit(6, _length(6))


def test_host_pointers_from_four_threads(eng, expected):
    plan = {t: [30 + 6 * t + i for i in range(6)] for t in range(4)}  # three commitments, three openings each
    wanted = {}
    for t, seeds in plan.items():
        for i, sd in enumerate(seeds):
            n = MIN_N + 211 * (sd - 30)
            wanted[sd] = (n, expected.commit(sd, n) if i < 3 else expected.opening(sd, n))
    results, errors = {}, []

    def work(t):
        try:
            for i, sd in enumerate(plan[t]):
                n, w = wanted[sd]
                if i < 3:
                    results[sd] = eng.commit_limbs(_poly(sd, n)).compress()
                else:
                    results[sd] = eng.open_limbs(_poly(sd, n), w[0], w[1]).compress()
        except Exception as e:  # (reported by the main thread)
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in plan]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t, seeds in plan.items():
        for i, sd in enumerate(seeds):
            n, w = wanted[sd]
            assert results[sd] == (w if i < 3 else w[2]), (t, i)


def test_new_srs_under_the_same_context(expected):
    e = K.Engine(0)
    try:
        e.srs_generate(SECRET, SRS_N)
        with _Resident(e) as dev:
            for s in range(e.num_slots()):
                e.commit_submit(s, dev.put(_poly(s, _length(s))), _length(s))
            for s in range(e.num_slots()):
                assert e.wait(s).compress() == expected.commit(s, _length(s))
        e.srs_generate(SECRET, MIN_N)
        assert e.srs_len() == MIN_N
        with _Resident(e) as dev:
            lens = [MIN_N - 3 * s for s in range(e.num_slots())]
            for s, n in enumerate(lens):
                e.commit_submit(s, dev.put(_poly(50 + s, n)), n)
            for s, n in reversed(list(enumerate(lens))):
                assert e.wait(s).compress() == expected.commit(50 + s, n, MIN_N)
    finally:
        e.close()  # nothing in flight
