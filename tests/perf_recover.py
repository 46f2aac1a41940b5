"""Recovery (kzg_recover_cells_and_proofs) at the DAS shape (4096, 8192, 64) with 64 random cells received, batches 1, 8 and 64,
and at (4096, 8192, 1) with half of the cells missing: the coefficients-only call, the full call (cells and proofs) and
kzg_cells_and_proofs_fk20 with cells on the same original polynomials, in the same run.  GPU; writes JSON lines to
profiles/r08_recover.jsonl (or the path given) and prints them."""
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
import oracle_ctypes as O  # noqa: E402  (bench inputs only)

REPS = int(os.environ.get("KZG_PERF_REPS", "5"))


def median_time(fn, reps):
    fn()  # warm
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def polys(n, batch):
    base = np.ascontiguousarray(O.bench_coefficients(n), dtype=np.uint64).reshape(n, 4)
    out = np.repeat(base[None], batch, axis=0)
    out[:, 0, 0] = np.arange(batch, dtype=np.uint64) + 1  # distinct polynomials
    return out


def shape(eng, n, log_n, log_l, k, batches):
    M = 1 << (log_n - log_l)
    recs = []
    for b in batches:
        c = polys(n, b)
        cells, _ = eng.cells_and_proofs_fk20(c, log_n, log_l)
        ids = random.Random(b).sample(range(M), k)
        rx = np.ascontiguousarray(cells.reshape(b, M, 1 << log_l, 4)[:, ids])
        co, _, _ = eng.recover_cells_and_proofs(n, log_n, log_l, ids, rx, cells_out=False, proofs=False)
        assert np.array_equal(co, c)
        t_coef = median_time(lambda: eng.recover_cells_and_proofs(n, log_n, log_l, ids, rx, cells_out=False, proofs=False), REPS)
        t_full = median_time(lambda: eng.recover_cells_and_proofs(n, log_n, log_l, ids, rx, coeffs=False), REPS)
        t_fk20 = median_time(lambda: eng.cells_and_proofs_fk20(c, log_n, log_l), REPS)
        rec = {"n": n, "N": 1 << log_n, "l": 1 << log_l, "received": k, "batch": b,
               "coeffs_ms": round(1e3 * t_coef, 3), "coeffs_polys_per_s": round(b / t_coef, 1),
               "full_ms": round(1e3 * t_full, 3), "fk20_cells_ms": round(1e3 * t_fk20, 3),
               "full_over_fk20": round(t_full / t_fk20, 3)}
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    return recs


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r08_recover.jsonl")
    eng = K.SetupArtifactsGenerator(bytes(range(32))).take(4096)
    try:
        eng.fk20_prepare(4096, 6)
        with open(out, "w") as f:
            for n, log_n, log_l, k, batches in ((4096, 13, 6, 64, [1, 8, 64]), (4096, 13, 0, 4096, [1, 8])):
                for rec in shape(eng, n, log_n, log_l, k, batches):
                    f.write(json.dumps(rec) + "\n")
    finally:
        eng.close()


if __name__ == "__main__":
    main()
