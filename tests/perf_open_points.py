"""Multiproofs at degree 2^20: proofs/s and points proven/s through kzg_open_points_submit / kzg_wait with every slot in
flight, the quotient's own time (kzg_get_times), and kzg_open's pipelined rate in the same run.  GPU; prints JSON lines."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import kzg_poly_commit_exploration_amd as K  # noqa: E402
import oracle_ctypes as O  # noqa: E402  (bench inputs only)


def pipelined(eng, submit, reps):
    slots = eng.num_slots()
    for phase in ("warm", "timed"):
        count = 10 if phase == "warm" else reps
        t0 = time.perf_counter()
        inflight = []
        for i in range(count):
            s = i % slots
            if len(inflight) == slots:
                eng.wait(inflight.pop(0))
            submit(s)
            inflight.append(s)
        while inflight:
            eng.wait(inflight.pop(0))
        dt = time.perf_counter() - t0
    return reps / dt


def main():
    degree = 1 << 20
    n = degree + 1
    reps = int(os.environ.get("KZG_PERF_REPS", "60"))
    eng = K.SetupArtifactsGenerator(bytes(range(32))).take(n)
    c = O.bench_coefficients(n)
    d = eng.dev_alloc(n * 32)
    eng.dev_upload(d, np.ascontiguousarray(c))
    z0 = K.Scalar.from_limbs(O.bench_input_point(degree))
    y0 = eng.evaluate_limbs(c, z0)
    open_rate = pipelined(eng, lambda s: eng.open_submit(s, d, n, z0, y0), reps)
    for k in (1, 2, 4, 8, 16, 32, 64):
        zs = [K.Scalar(z0.v + i) for i in range(k)]
        ys = eng.evaluate_points_limbs(c, zs)
        rate = pipelined(eng, lambda s: eng.open_points_submit(s, d, n, zs, ys), reps)
        eng.set_timing(True)  # one job alone for the quotient's own span
        eng.open_points_submit(0, d, n, zs, ys)
        eng.wait(0)
        quotient_ms = eng.times(0)["quotient_ms"]
        eng.set_timing(False)
        print(json.dumps({"degree": degree, "k": k, "proofs_per_s": round(rate, 2), "points_per_s": round(rate * k, 1),
                          "quotient_ms": round(quotient_ms, 4), "quotient_us_per_root": round(1e3 * quotient_ms / k, 2),
                          "open_proofs_per_s": round(open_rate, 2),
                          "points_vs_open": round(rate * k / open_rate, 2)}), flush=True)
    eng.dev_free(d)
    eng.close()


if __name__ == "__main__":
    main()
