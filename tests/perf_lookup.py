"""The log-derivative lookup calls (DESIGN.md sections 4.21 and 5.0r) on one device, one process, warmed, KZG_PERF_REPS
repetitions each (default 3) with their min-max, at n = 2^KZG_PERF_LOG_N (default 20):
  (a) the lookup form's running sum at k = 1, 3, 7 lookup columns: wall time of the synchronous device-pointer call (it returns
      when phi is in the caller's buffer: three kernels and one stream synchronise) and of the host-pointer call (uploads and the
      copy back included); the algorithmic bytes of the two streaming kernels -- k_lu_tile_lookup reads k + 2 columns and writes
      one, k_lu_finish reads and writes one: (k + 5) x 32 x n -- over the device call's time, against the copy rate of
      profiles/r21_microbench_copy.json;
  (b) the route without the calls: tests/host/lu_cpu_port.cpp (g++ -O2 over host_fr.hpp, Montgomery's trick, 16 threads) plus the
      copies it implies, measured here: k + 2 columns down from the device, phi up again -- a PORT for scale, not a tuned library;
  (c) kzg_lookup_multiplicities_device at n_table = n, k = 3 for uniform lookups, every lookup on one row, and a table whose
      images are 0, 1, 2, ..; the same through std::unordered_map in the port (built by one thread, probed by 16).
`--kernels`: only a few device calls per shape, for a separate `rocprofv3 --kernel-trace --stats` run (the kernels' own times;
k_lu_carry holds the call's one inversion and its serial scans: the latency floor of a call).
GPU.  Writes JSON lines to profiles/r22_logup.jsonl (or the path given) and prints them."""
import ctypes as C
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
R = K.R_MODULUS
COPY_RATE = 5797.7e9  # bytes / s: profiles/r21_microbench_copy.json
COLUMNS = (1, 3, 7)
KM = 3  # lookup columns of the multiplicities


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


def cpu_port(*args):
    exe = os.path.join(tempfile.mkdtemp(prefix="lu_cpu_"), "lu_cpu_port")
    subprocess.run(["g++", "-O2", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "host", "lu_cpu_port.cpp")], check=True,
                   stderr=subprocess.DEVNULL)
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout.split()
    return stats([float(v) for v in out[:REPS]])


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    kernels_only = "--kernels" in sys.argv
    out = args[0] if args else os.path.join(ROOT, "profiles", "r22_logup.jsonl")
    n = 1 << LOG_N
    eng = K.Engine(0)  # no call here needs an SRS
    lib = K.load_library()
    rng = np.random.default_rng(22)
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    kmax = max(COLUMNS)
    table = values(rng, n)
    looks = table[rng.integers(0, n, size=kmax * n)].reshape(kmax, n, 4)
    beta = K.Scalar(int(rng.integers(1, 1 << 62)) ** 4 % R)
    d_f, d_t, d_m, d_phi = eng.dev_alloc(kmax * n * 32), eng.dev_alloc(n * 32), eng.dev_alloc(n * 32), eng.dev_alloc(n * 32)
    host = np.zeros((kmax + 2, n, 4), dtype=np.uint64)
    try:
        eng.dev_upload(d_f, looks)
        eng.dev_upload(d_t, table)
        shapes = {"uniform": (table, looks[:KM]),
                  "one_row": (table, np.ascontiguousarray(np.broadcast_to(table[77], (KM, n, 4)))),
                  "small_images": (np.ascontiguousarray(np.pad(np.arange(n, dtype=np.uint64)[:, None], ((0, 0), (0, 3)))), None)}
        small = shapes["small_images"][0]
        shapes["small_images"] = (small, small[rng.integers(0, n, size=KM * n)].reshape(KM, n, 4))
        for name, (tb, lk) in shapes.items():
            eng.dev_upload(d_t, tb)
            eng.dev_upload(d_f, lk)
            call = lambda: eng.lookup_multiplicities_device(d_t, n, d_f, n, KM, d_m)
            if kernels_only:
                for _ in range(4):
                    call()
                continue
            call()  # warm
            emit({"what": "lookup_multiplicities", "measured": True, "lookups": name, "log_n_table": LOG_N, "log_n": LOG_N, "k": KM,
                  "reps": REPS, "device_call": stats([timed(call) for _ in range(REPS)]),
                  "host_call": stats([timed(lambda: eng.lookup_multiplicities(tb, lk, want_rows=False)) for _ in range(REPS)])})
        # the sums: the multiplicities of the uniform lookups are in place for k = 3; any m serves the timing of the others
        eng.dev_upload(d_t, table)
        eng.dev_upload(d_f, looks)
        mult, _ = eng.lookup_multiplicities(table, looks[:KM], want_rows=False)
        eng.dev_upload(d_m, mult)
        for k in COLUMNS:
            dev = lambda: eng.lookup_sum_device(d_f, n, k, d_t, d_m, beta, d_phi)
            if kernels_only:
                for _ in range(4):
                    dev()
                continue
            hst = lambda: eng.lookup_sum_limbs(looks[:k], table, mult, beta)
            last = dev()
            hst()  # warm
            sd = stats([timed(dev) for _ in range(REPS)])
            nbytes = (k + 5) * 32 * n
            rate = nbytes / (sd["median_ms"] * 1e-3)

            def copies():  # what the route without the call moves: k + 2 columns down, phi up
                for j in range(k):
                    assert lib.kzg_dev_download(eng._h, host[j].ctypes.data, C.c_void_p(d_f + j * n * 32), n * 32) == 0
                assert lib.kzg_dev_download(eng._h, host[k].ctypes.data, C.c_void_p(d_t), n * 32) == 0
                assert lib.kzg_dev_download(eng._h, host[k + 1].ctypes.data, C.c_void_p(d_m), n * 32) == 0
                eng.dev_upload(d_phi, host[0])

            copies()
            emit({"what": "lookup_sum", "measured": True, "log_n": LOG_N, "k": k, "reps": REPS, "device_call": sd,
                  "host_call": stats([timed(hst) for _ in range(REPS)]), "last_is_zero": bool(k == KM and not np.any(last)),
                  "streaming_bytes": nbytes, "bytes_per_s": round(rate, 1), "share_of_copy_rate": round(rate / COPY_RATE, 4),
                  "copies_without_the_call": stats([timed(copies) for _ in range(REPS)])})
    finally:
        for d in (d_f, d_t, d_m, d_phi):
            eng.dev_free(d)
        eng.close()
    if kernels_only:
        return
    for k in COLUMNS:
        emit({"what": "cpu_port_sum", "measured": True, "label": "a port to host_fr.hpp, g++ -O2, 16 threads: for scale only",
              "log_n": LOG_N, "k": k, "reps": REPS, "threads_16": cpu_port("sum", LOG_N, k, 16, REPS)})
    for dist, name in enumerate(("uniform", "one_row", "small_images")):
        emit({"what": "cpu_port_multiplicities", "measured": True, "label": "std::unordered_map built by one thread, probed by 16",
              "lookups": name, "log_n": LOG_N, "k": KM, "reps": REPS, "threads_16": cpu_port("mult", LOG_N, KM, 16, REPS, dist)})
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
