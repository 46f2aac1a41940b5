"""The grand product (DESIGN.md sections 4.19 and 5.0p) on one device, one process, warmed, KZG_PERF_REPS repetitions each
(default 3) with their min-max, at n = 2^KZG_PERF_LOG_N (default 20) and t = 1, 3, 5 columns per side, general and permutation
form:
  (a) wall time of the synchronous device-pointer call (it returns when z is in the caller's buffer: three kernels and one
      stream synchronise), of the host-pointer call (uploads and the copy back included) and of kzg_permutation_commit;
      the algorithmic bytes (2 t + 3) x 32 x n over the device call's time as a fraction of the HBM figures;
  (b) the same z on the CPU: tests/host/gp_cpu_port.cpp (g++ -O2 over host_fr.hpp, Montgomery's trick) on 1 and 16 threads --
      a PORT for scale, not a tuned CPU library.
`--kernels`: only a few device calls per shape, for a separate `rocprofv3 --kernel-trace --stats` run (the three kernels' own
times; k_gp_carry holds the call's one inversion and two serial scans: the latency floor of a call).
GPU.  Writes JSON lines to profiles/r20_grand_product.jsonl (or the path given) and prints them."""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import kzg_poly_commit_exploration_amd as K  # noqa: E402

REPS = max(int(os.environ.get("KZG_PERF_REPS", "3")), 3)
LOG_N = int(os.environ.get("KZG_PERF_LOG_N", "20"))
SECRET = bytes(range(32))
R = K.R_MODULUS
HBM_SPEC, HBM_MEASURED = 8.0e12, 6.29e12  # bytes / s: the data sheet, and a float4 copy on this part
COLUMNS = (1, 3, 5)


def stats(ts, scale=1e3, unit="ms"):
    return {"median_" + unit: round(scale * float(np.median(ts)), 4), "min_" + unit: round(scale * min(ts), 4),
            "max_" + unit: round(scale * max(ts), 4)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def values(rng, rows):
    a = rng.integers(1, 1 << 64, size=(rows, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, R >> 192, size=rows, dtype=np.uint64)
    return a


def cpu_port(log_n, t, threads):
    exe = os.path.join(tempfile.mkdtemp(prefix="gp_cpu_"), "gp_cpu_port")
    subprocess.run(["g++", "-O2", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "host", "gp_cpu_port.cpp")], check=True,
                   stderr=subprocess.DEVNULL)
    out = subprocess.run([exe, str(log_n), str(t), str(threads), str(REPS)], capture_output=True, text=True, check=True).stdout.split()
    return stats([float(v) for v in out[:REPS]])


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    kernels_only = "--kernels" in sys.argv
    out = args[0] if args else os.path.join(ROOT, "profiles", "r20_grand_product.jsonl")
    n = 1 << LOG_N
    eng = K.Engine(0) if kernels_only else K.SetupArtifactsGenerator(SECRET).take(n)  # only the commitment needs an SRS
    rng = np.random.default_rng(20)
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    tmax = max(COLUMNS)
    a, b = values(rng, tmax * n).reshape(tmax, n, 4), values(rng, tmax * n).reshape(tmax, n, 4)
    shifts = [K.Scalar(pow(7, j, R)) for j in range(tmax)]
    beta, gamma = K.Scalar(int(rng.integers(1, 1 << 62)) ** 4 % R), K.Scalar(int(rng.integers(1, 1 << 62)) ** 4 % R)
    d_a, d_b, d_z = eng.dev_alloc(tmax * n * 32), eng.dev_alloc(tmax * n * 32), eng.dev_alloc(n * 32)
    try:
        eng.dev_upload(d_a, a)
        eng.dev_upload(d_b, b)
        for t in COLUMNS:
            calls = {
                "general": (lambda: eng.grand_product_device(d_a, d_b, n, t, d_z),
                            lambda: eng.grand_product_limbs(a[:t], b[:t])),
                "permutation": (lambda: eng.permutation_product_device(d_a, d_b, n, t, shifts[:t], beta, gamma, d_z),
                                lambda: eng.permutation_product_limbs(a[:t], b[:t], shifts[:t], beta, gamma)),
            }
            for form, (dev, host) in calls.items():
                if kernels_only:
                    for _ in range(4):
                        dev()
                    continue
                dev(), host()  # warm
                td, th = [timed(dev) for _ in range(REPS)], [timed(host) for _ in range(REPS)]
                sd = stats(td)
                nbytes = (2 * t + 3) * 32 * n
                rate = nbytes / (sd["median_ms"] * 1e-3)
                emit({"what": "grand_product", "measured": True, "form": form, "log_n": LOG_N, "t": t, "reps": REPS,
                      "device_call": sd, "host_call": stats(th), "algorithmic_bytes": nbytes,
                      "bytes_per_s": round(rate, 1), "share_of_hbm_spec": round(rate / HBM_SPEC, 4),
                      "share_of_hbm_measured": round(rate / HBM_MEASURED, 4)})
            if kernels_only:
                continue
            commit = lambda: eng.permutation_commit(a[:t], b[:t], shifts[:t], beta, gamma, want_z=False)
            commit()  # builds the basis on first use, warms
            emit({"what": "permutation_commit", "measured": True, "log_n": LOG_N, "t": t, "reps": REPS,
                  "call": stats([timed(commit) for _ in range(REPS)])})
    finally:
        for d in (d_a, d_b, d_z):
            eng.dev_free(d)
        eng.close()
    if kernels_only:
        return
    for t in COLUMNS:
        emit({"what": "cpu_port", "measured": True, "label": "a port of the algorithm to host_fr.hpp, g++ -O2: for scale only",
              "log_n": LOG_N, "t": t, "reps": REPS, "threads_1": cpu_port(LOG_N, t, 1), "threads_16": cpu_port(LOG_N, t, 16)})
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
