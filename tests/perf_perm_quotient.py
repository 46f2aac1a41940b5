"""The quotient of a permutation argument (DESIGN.md sections 4.20 and 5.0q) on one device, one process, warmed,
KZG_PERF_REPS repetitions each (default 3) with their min-max, at n = 2^16, 2^18, 2^20 (KZG_PERF_LOGS), t = 3, e = 4:
  (a) wall time of kzg_permutation_quotient (uploads, T's coefficients and the three commitments back) and of the same call
      without the coefficients;
  (b) the route a caller has without it, step by step: kzg_ntt per column down to coefficients (2 t + 1 calls at n) and up
      to the coset (2 t + 2 calls at N, L_0 included), the pointwise work on the host (tests/host/pq_cpu_port.cpp, g++ -O2 over
      host_fr.hpp, 16 threads: twist, constraints, untwist -- a PORT for scale, not a tuned CPU library), kzg_ntt back at N,
      kzg_commit_batch of the three chunks; their sum;
  (c) the phases of the composite as device-pointer calls, each returning after one stream synchronise: kzg_coset_extend_device of
      the 2 t + 1 columns, kzg_permutation_constraints_coset_device (L_0's extension, the upload of the e inverses and
      k_pq_constraints), kzg_vanishing_quotient_device (inverse transform, untwist), kzg_commit_batch of the chunks;
  (d) with the copy rate given as KZG_COPY_GBS (tools/microbench copy on the same box): the time (2 t + 4) x 32 bytes read and 32
      written per point take at that rate, for the ratio with k_pq_constraints' own time.
`--kernels`: a few composite calls per size and nothing else, for a separate `rocprofv3 --kernel-trace --stats` run (the
kernels' own times).
GPU.  Writes JSON lines to profiles/r21_perm_quotient.jsonl (or the path given) and prints them."""
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
LOGS = [int(v) for v in os.environ.get("KZG_PERF_LOGS", "16,18,20").split(",")]
COPY_GBS = float(os.environ.get("KZG_COPY_GBS", "0"))
SECRET = bytes(range(32))
R = K.R_MODULUS
T, LOG_EXT = 3, 2


def stats(ts, scale=1e3, unit="ms"):
    return {"median_" + unit: round(scale * float(np.median(ts)), 4), "min_" + unit: round(scale * min(ts), 4),
            "max_" + unit: round(scale * max(ts), 4)}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def measure(fn):
    fn()  # warm
    return stats([timed(fn) for _ in range(REPS)])


def values(rng, rows):
    a = rng.integers(1, 1 << 64, size=(rows, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, R >> 192, size=rows, dtype=np.uint64)
    return a


def cpu_port(log_n, threads):
    exe = os.path.join(tempfile.mkdtemp(prefix="pq_cpu_"), "pq_cpu_port")
    subprocess.run(["g++", "-O2", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "host", "pq_cpu_port.cpp")], check=True,
                   stderr=subprocess.DEVNULL)
    out = subprocess.run([exe, str(log_n), str(LOG_EXT), str(T), str(threads), str(REPS)], capture_output=True, text=True,
                         check=True).stdout.split("\n")
    rows = [[float(v) for v in line.split()] for line in out[:REPS]]
    return {"twist": stats([r[0] for r in rows]), "constraints": stats([r[1] for r in rows]), "untwist": stats([r[2] for r in rows]),
            "total": stats([sum(r) for r in rows])}


def cyclic_argument(eng, n, rng):
    """wires equal across the t columns of a row and the permutation (j, i) -> (j + 1 mod t, i): a true permutation at any size,
    made with vector operations only; z from kzg_permutation_product"""
    row = values(rng, n)
    wires = np.stack([row] * T)
    shifts = [K.Scalar(pow(7, j, R)) for j in range(T)]
    sig = []
    for j in range(T):  # k_(j+1) w^i: the values of the polynomial k_(j+1) X
        c = np.zeros((n, 4), dtype=np.uint64)
        c[1] = shifts[(j + 1) % T].limbs()
        sig.append(eng.ntt_limbs(c))
    return wires, np.stack(sig), shifts


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    kernels_only = "--kernels" in sys.argv
    out = args[0] if args else os.path.join(ROOT, "profiles", "r21_perm_quotient.jsonl")
    eng = K.SetupArtifactsGenerator(SECRET).take(1 << max(LOGS))
    eng.set_max_batch((1 << LOG_EXT) - 1)  # the chunks of T go through one batched MSM, in the call and in the route without it
    rng = np.random.default_rng(21)
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    alpha, beta, gamma = (K.Scalar(int(rng.integers(1, 1 << 62)) ** 4 % R) for _ in range(3))
    try:
        for log_n in LOGS:
            n, e = 1 << log_n, 1 << LOG_EXT
            N, ncols = n * e, 2 * T + 1
            wires, sigmas, shifts = cyclic_argument(eng, n, rng)
            z, last = eng.permutation_product_limbs(wires, sigmas, shifts, beta, gamma)
            assert [int(x) for x in last] == [int(x) for x in K.Scalar(1).limbs()]
            full = lambda: eng.permutation_quotient(wires, sigmas, z, shifts, alpha, beta, gamma, LOG_EXT)
            if kernels_only:
                for _ in range(4):
                    full()
                continue
            emit({"what": "permutation_quotient", "measured": True, "log_n": log_n, "t": T, "log_ext": LOG_EXT, "reps": REPS,
                  "call": measure(full),
                  "call_without_coefficients": measure(lambda: eng.permutation_quotient(wires, sigmas, z, shifts, alpha, beta, gamma,
                                                                                        LOG_EXT, want_coeffs=False))})
            coeffs, points = full()
            # (b) the route without the call
            col_n, col_N = wires[0], values(rng, N)
            chunks = [coeffs[c * n:(c + 1) * n] for c in range(e - 1)]
            eng.commit_batch_limbs(chunks)
            down, up = measure(lambda: eng.intt_limbs(col_n)), measure(lambda: eng.ntt_limbs(col_N))
            back, msm = measure(lambda: eng.intt_limbs(col_N)), measure(lambda: eng.commit_batch_limbs(chunks))
            host = cpu_port(log_n, 16)
            total = (ncols * down["median_ms"] + (ncols + 1) * up["median_ms"] + host["total"]["median_ms"] + back["median_ms"] +
                     msm["median_ms"])
            emit({"what": "route_without_the_call", "measured": True, "log_n": log_n, "t": T, "log_ext": LOG_EXT, "reps": REPS,
                  "kzg_ntt_inverse_at_n": down, "calls_at_n": ncols, "kzg_ntt_at_N": up, "calls_at_N": ncols + 1,
                  "host_pointwise_16_threads": host, "kzg_ntt_inverse_at_N": back, "kzg_commit_batch_of_chunks": msm,
                  "sum_of_medians_ms": round(total, 3)})
            # (c) the phases as device calls
            d_in, d_ext = eng.dev_alloc(ncols * n * 32), eng.dev_alloc(ncols * N * 32)
            d_out, d_coef = eng.dev_alloc(N * 32), eng.dev_alloc(N * 32)
            try:
                eng.dev_upload(d_in, np.concatenate([wires.reshape(-1, 4), sigmas.reshape(-1, 4), z]))
                ext = measure(lambda: eng.coset_extend_device(d_in, n, ncols, log_n + LOG_EXT, d_ext))
                d_s, d_z = d_ext + T * N * 32, d_ext + 2 * T * N * 32
                con = measure(lambda: eng.permutation_constraints_coset_device(d_ext, d_s, d_z, n, e, T, shifts, alpha, beta, gamma, d_out))
                one = measure(lambda: eng.coset_extend_device(d_in, n, 1, log_n + LOG_EXT, d_coef, form=K.KZG_EXTEND_COEFFS))
                quo = measure(lambda: eng.vanishing_quotient_device(d_out, N, n, d_coef, already_divided=True))
            finally:
                for d in (d_in, d_ext, d_out, d_coef):
                    eng.dev_free(d)
            line = {"what": "phases_as_device_calls", "measured": True, "log_n": log_n, "t": T, "log_ext": LOG_EXT, "reps": REPS,
                    "extension_of_2t+1_columns": ext, "constraints_call": con, "extension_of_one_column_of_coefficients": one,
                    "inverse_transform_and_untwist": quo, "msm_of_chunks": msm}
            if COPY_GBS:
                nbytes = ((2 * T + 4) * 32 + 32) * N
                line.update({"copy_GBs": COPY_GBS, "constraints_bytes": nbytes, "constraints_bytes_at_copy_rate_ms": round(nbytes / COPY_GBS / 1e6, 4)})
            emit(line)
    finally:
        eng.close()
    if kernels_only:
        return
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
