"""Blob proofs from wire bytes against the same work chained by hand from the older entry points, at
n = 4096 in KZG_ORDER_BIT_REVERSED with 1 and 64 blobs per call, kzg_set_max_batch(64) for both legs:
  * quotients   quotient_ms (kzg_set_timing) of the batched kernel inside kzg_blobs_open_at_bytes for 64 polynomials, against
                quotient_ms of kzg_open_batch_submit on the same coefficients resident on the device: the per-polynomial loop;
  * proofs      kzg_blobs_to_blob_proofs_bytes (commitments computed) against hashlib, kzg_fr_from_bytes_batch, kzg_ntt per blob,
                kzg_commit_batch, kzg_evaluate_evaluations_batch, kzg_open_batch and kzg_g1_compress per point;
  * verify      kzg_verify_blob_proofs_batch_bytes against hashlib and kzg_verify_blobs_batch_bytes;
  * hash        kzg_blob_challenges_bytes on one thread (KZG_HASH_THREADS=1) and on the pool, and hashlib on one thread.
Each figure is the median of KZG_PERF_REPS alternated calls (default 5) after a warm-up round; the script repeats that three
times and reports the median of the three with their minimum and maximum.  Outputs of the two legs are compared before timing.
GPU.  The process pins itself to 16 CPUs before anything starts a thread.  Writes JSON lines to
profiles/r17_blob_proofs.jsonl (or the path given) and prints them."""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kzg_poly_commit_exploration_amd as K  # noqa: E402

REPS = int(os.environ.get("KZG_PERF_REPS", "5"))
SECRET = bytes(range(32))
R = K.R_MODULUS
BRP = K.KZG_ORDER_BIT_REVERSED
N = 4096


def alternate(fns, reps):
    """medians (ms) of the given calls, run in turn `reps` times after one warm-up round"""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ts[i].append(1e3 * (time.perf_counter() - t0))
    return [float(np.median(t)) for t in ts]


def spread(values):
    return {"median": round(float(np.median(values)), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def brp_perm(bits):
    return np.array([int(format(i, "0%db" % bits)[::-1], 2) for i in range(1 << bits)], dtype=np.int64)


def challenges(blobs, coms):
    out = []
    for i, b in enumerate(blobs):
        d = hashlib.sha256(b"FSBLOBVERIFY_V1_" + N.to_bytes(16, "big") + b + coms[48 * i:48 * i + 48]).digest()
        out.append(int.from_bytes(d, "big") % R)
    return out


def main():
    os.sched_setaffinity(0, sorted(os.sched_getaffinity(0))[:16])
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r17_blob_proofs.jsonl")
    lib = K.load_library()
    recs = []

    def emit(rec):
        rec.update({"n": N, "order": "bit_reversed", "inner_reps": REPS, "repetitions": 3, "max_batch": 64})
        recs.append(rec)
        print(json.dumps(rec), flush=True)

    perm = brp_perm(12)
    g2 = np.ascontiguousarray(np.stack([K.srs_g2_at(SECRET, i) for i in range(2)]))
    eng = K.SetupArtifactsGenerator(SECRET).take(N)
    try:
        assert eng.set_max_batch(64) == 64
        rng = np.random.default_rng(17)
        for batch in (1, 64):
            raw = rng.integers(0, 256, size=(batch, N, 32), dtype=np.uint8)
            raw[:, :, 0] &= 0x3F  # every value below 2^254 < r
            blobs = [raw[b].tobytes() for b in range(batch)]
            data = b"".join(blobs)

            def hand_proofs():
                vals = eng.fr_from_bytes_batch(data).reshape(batch, N, 4)[:, perm]
                coeffs = np.stack([eng.intt_limbs(v) for v in vals])
                coms = b"".join(p.compress() for p in eng.commit_batch_host(coeffs))
                zs = [K.Scalar(z) for z in challenges(blobs, coms)]
                ys = eng.evaluate_evaluations_batch(vals, zs)
                proofs = b"".join(p.compress() for p in eng.open_batch_host(coeffs, zs, ys))
                return coms, proofs

            def new_proofs():
                return eng.blobs_to_blob_proofs_bytes(data, N, order=BRP)

            coms, proofs = new_proofs()
            assert hand_proofs() == (coms, proofs), "the two routes must give the same bytes"

            def hand_verify():
                zs_be = b"".join(z.to_bytes(32, "big") for z in challenges(blobs, coms))
                assert eng.verify_blobs_batch_bytes(data, N, coms, zs_be, proofs, g2, order=BRP, want_ys=False)[0]

            def new_verify():
                assert eng.verify_blob_proofs_batch_bytes(data, N, coms, proofs, g2, order=BRP)

            def hash_one():
                os.environ["KZG_HASH_THREADS"] = "1"
                K.blob_challenges_bytes(data, N, coms)
                del os.environ["KZG_HASH_THREADS"]

            def hash_pool():
                K.blob_challenges_bytes(data, N, coms)

            def hash_hashlib():
                challenges(blobs, coms)

            names = ("proofs_hand_ms", "proofs_new_ms", "verify_hand_ms", "verify_new_ms", "hash_1_thread_ms", "hash_pool_ms",
                     "hash_hashlib_1_thread_ms")
            runs = [alternate([hand_proofs, new_proofs, hand_verify, new_verify, hash_one, hash_pool, hash_hashlib], REPS)
                    for _ in range(3)]
            rec = {"what": "blob_proofs_calls", "blobs": batch}
            for i, name in enumerate(names):
                rec[name] = spread([r[i] for r in runs])
            rec["proofs_hand_over_new"] = round(rec["proofs_hand_ms"]["median"] / rec["proofs_new_ms"]["median"], 3)
            rec["verify_hand_over_new"] = round(rec["verify_hand_ms"]["median"] / rec["verify_new_ms"]["median"], 3)
            emit(rec)

            if batch != 64:
                continue
            # ---- the quotients alone: device events around the batched kernel and around the per-polynomial loop
            zs_int = challenges(blobs, coms)
            zs_be = b"".join(z.to_bytes(32, "big") for z in zs_int)
            vals = eng.fr_from_bytes_batch(data).reshape(batch, N, 4)[:, perm]
            coeffs = np.ascontiguousarray(np.stack([eng.intt_limbs(v) for v in vals]))
            zl = np.ascontiguousarray(K.scalars_to_limbs(zs_int))
            ys_be, _ = eng.blobs_open_at_bytes(data, N, zs_be, order=BRP)
            yl = np.ascontiguousarray(K.scalars_to_limbs([int.from_bytes(ys_be[32 * b:32 * b + 32], "big") for b in range(batch)]))
            dptr = eng.dev_alloc(coeffs.nbytes)
            eng.dev_upload(dptr, coeffs)
            out = np.zeros((batch, 18), dtype=np.uint64)
            st = np.zeros(batch, dtype=np.int32)
            P = K._ptr
            eng.set_timing(True)

            def q_loop():
                assert lib.kzg_open_batch_submit(eng._h, 0, K.C.c_void_p(dptr), N, batch, N, P(zl), P(yl)) == 0
                assert lib.kzg_wait_open_batch(eng._h, 0, P(out), P(st), batch) == 0 and not st.any()
                return eng.times(0)["quotient_ms"]

            def q_kernel():
                eng.blobs_open_at_bytes(data, N, zs_be, order=BRP)
                return max(eng.times(s)["quotient_ms"] for s in range(eng.num_slots()))

            loop_runs, kernel_runs = [], []
            for _ in range(3):
                q_loop(), q_kernel()
                a, b = [], []
                for _ in range(REPS):
                    a.append(q_loop())
                    b.append(q_kernel())
                loop_runs.append(float(np.median(a)))
                kernel_runs.append(float(np.median(b)))
            eng.set_timing(False)
            eng.dev_free(dptr)
            lp, kn = spread(loop_runs), spread(kernel_runs)
            emit({"what": "blob_proofs_quotients", "polynomials": batch, "loop_quotient_ms": lp, "kernel_quotient_ms": kn,
                  "loop_over_kernel": round(lp["median"] / kn["median"], 2) if kn["median"] else None,
                  "kernel_minus_loop_ms": round(kn["median"] - lp["median"], 4),
                  "loop_spread_ms": round(lp["max"] - lp["min"], 4),
                  "accepted": bool(kn["median"] - lp["median"] <= lp["max"] - lp["min"])})
    finally:
        eng.close()
        with open(out_path, "w") as f:
            for rec in recs:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
