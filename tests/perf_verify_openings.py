"""Openings at arbitrary points, old and new routes alternated call by call on the same inputs:
  * kzg_verify_openings_batch against kzg_verify_proof_batch (the host's cores) at k = 16 ... 65 536 records over 64
    commitments, every record at its own point and all records at one point;
  * kzg_evaluate_evaluations_batch against kzg_ntt(inverse) + kzg_evaluate per polynomial at (n, batch) = (4096, 64), (2^20, 1);
  * kzg_verify_evaluations_batch at (4096, 64) beside its two halves.
GPU; medians of KZG_PERF_REPS calls (default 20; the host route at 65 536 records takes seconds per call and gets
KZG_PERF_REPS_SLOW, default 3).  The process pins itself to KZG_PERF_HOST_CPUS CPUs (default 16) before anything starts a
thread, so both routes have that many cores whatever the box shows (KZG_PERF_HOST_CPUS=0: no pinning); kzg_verify_proof_batch starts
min(std::thread::hardware_concurrency(), k) threads, and every line records that count as the process sees it.  Writes JSON lines to profiles/r10_verify_openings.jsonl (or the path given) and prints
them.  The records are openings of polynomials of degree 1, a + b X: their quotient is b at every point, so one proof per
polynomial serves any number of distinct points -- the verifiers cannot tell and do the same work as for any other record."""
import ctypes
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kzg_poly_commit_exploration_amd as K  # noqa: E402

REPS = int(os.environ.get("KZG_PERF_REPS", "20"))
REPS_SLOW = int(os.environ.get("KZG_PERF_REPS_SLOW", "3"))
KS = [int(x) for x in os.environ.get("KZG_PERF_KS", "16,24,32,48,64,128,192,256,384,512,1024,4096,65536").split(",") if x]
ONLY_VERIFY = os.environ.get("KZG_PERF_ONLY_VERIFY") == "1"  # the verifier's lines only
HOST_CPUS = int(os.environ.get("KZG_PERF_HOST_CPUS", "16"))
SECRET = bytes(range(32))
R = K.R_MODULUS


def alternate(fns, reps):
    """medians (seconds) of the given calls, run in turn `reps` times after one warm-up round"""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ts[i].append(time.perf_counter() - t0)
    return [float(np.median(t)) for t in ts]


def images(rng, shape):
    a = rng.integers(0, 1 << 63, size=shape + (4,), dtype=np.uint64)
    a[..., 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
    return a


def main():
    if HOST_CPUS > 0:  # 0: no pinning, the process keeps every CPU the box shows it
        os.sched_setaffinity(0, sorted(os.sched_getaffinity(0))[:HOST_CPUS])
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r10_verify_openings.jsonl")
    g2 = [K.srs_g2_at(SECRET, i) for i in range(2)]
    eng = K.SetupArtifactsGenerator(SECRET).take(4096)
    lib = K.load_library()
    # what kzg_verify_proof_batch sizes its pool by, asked of the same C++ runtime after the pinning
    hw = ctypes.CDLL("libstdc++.so.6")._ZNSt6thread20hardware_concurrencyEv
    hw.restype = ctypes.c_uint
    hw_threads = int(hw()) or 1
    pinned = len(os.sched_getaffinity(0))
    recs = []

    def emit(rec):
        recs.append(rec)
        print(json.dumps(rec), flush=True)

    try:
        rnd = random.Random(1)
        B = 64
        ab = [(rnd.randrange(R), rnd.randrange(R)) for _ in range(B)]
        limbs = [K.scalars_to_limbs(list(c)) for c in ab]
        coms = np.stack([eng.commit_limbs(l).p1 for l in limbs])
        prfs = np.stack([eng.open_limbs(l, K.Scalar(3), K.Scalar((a + 3 * b) % R)).p1 for l, (a, b) in zip(limbs, ab)])
        for k in KS:
            for layout in ("distinct", "one"):
                idx = np.array([rnd.randrange(B) for _ in range(k)], dtype=np.uint32)
                z0 = rnd.randrange(R)
                zs = [z0 if layout == "one" else rnd.randrange(R) for _ in range(k)]
                ys = [(ab[b][0] + ab[b][1] * z) % R for b, z in zip(idx, zs)]
                zl, yl = K.scalars_to_limbs(zs), K.scalars_to_limbs(ys)
                cs, ps = np.ascontiguousarray(coms[idx]), np.ascontiguousarray(prfs[idx])
                ok = np.zeros(k, dtype=np.int32)
                s_g2 = np.ascontiguousarray(g2[1])

                def host():
                    rc = lib.kzg_verify_proof_batch(K._ptr(cs), K._ptr(ps), K._ptr(zl), K._ptr(yl), K._ptr(s_g2), k, K._ptr(ok))
                    assert rc == 0 and ok.all()

                def device():
                    assert eng.verify_openings_batch(coms, idx, zl, yl, prfs[idx], g2)

                reps = REPS if k <= 4096 else REPS_SLOW
                t_host, t_dev = alternate([host, device], reps)
                emit({"what": "verify_openings_batch", "records": k, "commitments": B, "points": layout, "reps": reps,
                      "host_cpus_pinned": pinned, "hardware_concurrency": hw_threads, "host_threads_started": min(hw_threads, k),
                      "verify_proof_batch_ms": round(1e3 * t_host, 3),
                      "verify_openings_batch_ms": round(1e3 * t_dev, 3), "speedup": round(t_host / t_dev, 2)})
        rng = np.random.default_rng(2)
        for n, batch in ((4096, 64), (1 << 20, 1)) if not ONLY_VERIFY else ():
            ev = images(rng, (batch, n))
            zs = K.scalars_to_limbs([rnd.randrange(R) for _ in range(batch)])
            zsc = [K.Scalar.from_limbs(z) for z in zs]

            def old():
                return [eng.evaluate_limbs(eng.intt_limbs(ev[b]), zsc[b]) for b in range(batch)]

            def new():
                return eng.evaluate_evaluations_batch(ev, zs)

            assert [v.v for v in old()] == [v.v for v in new()]
            t_old, t_new = alternate([old, new], REPS)
            emit({"what": "evaluate_evaluations_batch", "n": n, "batch": batch, "reps": REPS,
                  "ntt_inverse_plus_evaluate_ms": round(1e3 * t_old, 3), "evaluate_evaluations_batch_ms": round(1e3 * t_new, 3),
                  "speedup": round(t_old / t_new, 2)})
        if ONLY_VERIFY:
            return
        n, batch = 4096, 64
        ev = images(rng, (batch, n))
        zsc = [K.Scalar(rnd.randrange(R)) for _ in range(batch)]
        zs = np.stack([z.limbs() for z in zsc])
        ys = eng.evaluate_evaluations_batch(ev, zs)
        yl = np.stack([y.limbs() for y in ys])
        cm = np.stack([eng.commit_evaluations_limbs(ev[b]).p1 for b in range(batch)])
        pf = np.stack([eng.open_evaluations_limbs(ev[b], zsc[b], ys[b]).p1 for b in range(batch)])
        idx = np.arange(batch, dtype=np.uint32)

        def both():
            ok, _ = eng.verify_evaluations_batch(ev, cm, zs, pf, g2)
            assert ok

        def half_eval():
            eng.evaluate_evaluations_batch(ev, zs)

        def half_verify():
            assert eng.verify_openings_batch(cm, idx, zs, yl, pf, g2)

        t_both, t_e, t_v = alternate([both, half_eval, half_verify], REPS)
        emit({"what": "verify_evaluations_batch", "n": n, "batch": batch, "reps": REPS, "verify_evaluations_batch_ms": round(1e3 * t_both, 3),
              "evaluate_evaluations_batch_ms": round(1e3 * t_e, 3), "verify_openings_batch_ms": round(1e3 * t_v, 3),
              "sum_of_halves_ms": round(1e3 * (t_e + t_v), 3)})
    finally:
        eng.close()
        with open(out, "w") as f:
            for rec in recs:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
