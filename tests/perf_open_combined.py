"""Combined openings at n = 2^20 on resident inputs, t = 1, 4, 16, 64 polynomials at one point, per t:
  * combined_ms        kzg_open_combined_submit + kzg_wait_combined, host wall time;
  * loop_ms            the existing route for the same statement in the same process and run: t x kzg_open_submit through the
                       stream slots, as bench.py drives its openings (the claims are the values the combined call returned);
  * combine_kernel_ms  k_combine_eval and its finish kernel alone (kzg_set_timing / kzg_get_combine_ms: events around the two
                       launches), with its algorithmic bytes (t + 1) n 32 per second as a fraction of the 6.3 TB/s of HBM
                       bandwidth that is achievable on the MI355X; scan_ms / msm_ms: the rest of the job from kzg_get_times.
And the host-pointer call kzg_open_combined at t = 16 (pageable host memory: bound by the upload, 32 MiB per polynomial).
GPU; medians of KZG_PERF_REPS runs (default 3) after one warm-up run.  Writes JSON lines to profiles/r14_open_combined.jsonl (or
the path given) and prints them."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import kzg_poly_commit_exploration_amd as K  # noqa: E402

REPS = int(os.environ.get("KZG_PERF_REPS", "3"))
TS = [int(x) for x in os.environ.get("KZG_PERF_TS", "1,4,16,64").split(",") if x]
LOG_N = int(os.environ.get("KZG_PERF_LOG_N", "20"))
DISTINCT = 16  # different polynomials on the host; polynomial i of the block is number i mod DISTINCT
SECRET = bytes(range(32))
R = K.R_MODULUS
HBM_ACHIEVABLE = 6.3e12


def median_ms(fn, reps=REPS):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r14_open_combined.jsonl")
    n = 1 << LOG_N
    eng = K.SetupArtifactsGenerator(SECRET).take(n)
    rng = np.random.default_rng(14)
    host = rng.integers(0, 1 << 64, size=(DISTINCT, n, 4), dtype=np.uint64)
    host[..., 3] = rng.integers(0, R >> 192, size=(DISTINCT, n), dtype=np.uint64)
    z, gamma = K.Scalar(int(rng.integers(1, 1 << 62)) ** 4 % R), K.Scalar(int(rng.integers(1, 1 << 62)) ** 4 % R)
    tmax = max(TS)
    dptr = eng.dev_alloc(tmax * n * 32)
    lines = []
    try:
        for i in range(tmax):
            eng.dev_upload(dptr + i * n * 32, host[i % DISTINCT])
        slots = eng.num_slots()
        for t in TS:
            eng.set_timing(False)
            state = {}

            def combined():
                eng.open_combined_submit(0, dptr, n, t, z, gamma)
                state["ys"], state["pi"] = eng.wait_combined(0, t)

            combined_ms = median_ms(combined)
            ys = state["ys"]

            def loop():
                inflight, proofs = [], []
                for i in range(t):
                    slot = i % slots
                    if len(inflight) == slots:
                        proofs.append(eng.wait(inflight.pop(0)))
                    eng.open_submit(slot, dptr + i * n * 32, n, z, ys[i])
                    inflight.append(slot)
                while inflight:
                    proofs.append(eng.wait(inflight.pop(0)))
                state["proofs"] = proofs

            loop_ms = median_ms(loop)
            # the two routes prove the same statement: sum gamma^i proof_i is the combined proof (the quotient is linear in P)
            eng.set_timing(True)
            kernel, scan, msm = [], [], []
            for _ in range(REPS + 1):
                combined()
                kernel.append(eng.combine_ms(0))
                tm = eng.times(0)
                scan.append(tm["quotient_ms"])
                msm.append(tm["total_ms"] - tm["quotient_ms"])
            eng.set_timing(False)
            kernel_ms = float(np.median(kernel[1:]))
            bytes_alg = (t + 1) * n * 32
            rate = bytes_alg / (kernel_ms * 1e-3)
            lines.append({"what": "open_combined_resident", "log_n": LOG_N, "t": t, "reps": REPS,
                          "combined_ms": round(combined_ms, 4), "loop_ms": round(loop_ms, 4),
                          "loop_over_combined": round(loop_ms / combined_ms, 3),
                          "combine_kernel_ms": round(kernel_ms, 4), "scan_ms": round(float(np.median(scan[1:])), 4),
                          "msm_ms": round(float(np.median(msm[1:])), 4), "combine_bytes": bytes_alg,
                          "combine_tb_per_s": round(rate / 1e12, 4), "fraction_of_achievable_hbm": round(rate / HBM_ACHIEVABLE, 4)})
            print(json.dumps(lines[-1]), flush=True)
        t = 16
        if t <= tmax:
            block = np.ascontiguousarray(np.stack([host[i % DISTINCT] for i in range(t)]))
            for mb in (1, 4):
                eng.set_max_batch(mb)
                host_ms = median_ms(lambda: eng.open_combined_limbs(block, z, gamma))
                lines.append({"what": "open_combined_host_pointer", "log_n": LOG_N, "t": t, "reps": REPS, "max_batch": mb,
                              "host_call_ms": round(host_ms, 4), "uploaded_bytes": t * n * 32,
                              "upload_gb_per_s_if_all_upload": round(t * n * 32 / (host_ms * 1e-3) / 1e9, 3),
                              "note": "upload-bound: pageable host memory, one hipMemcpyAsync per pass, passes not overlapped"})
                print(json.dumps(lines[-1]), flush=True)
            eng.set_max_batch(1)
    finally:
        eng.dev_free(dptr)
        eng.close()
    with open(out, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
