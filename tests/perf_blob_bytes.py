"""The producing side on blob bytes against the route the existing entry points give, legs alternated
call by call on the same blobs, at the DAS shape (n = 4096, log_domain 13, log_cell 6, KZG_ORDER_BIT_REVERSED), 64 blobs per
call and 1 blob per call, SRS of 4096 points, FK20 tables prepared beforehand:
  * t_route  kzg_fr_from_bytes_batch on all values, the bit reversal undone with numpy, kzg_ntt per blob, kzg_commit_batch and
             kzg_cells_and_proofs_fk20 on the coefficient arrays, kzg_g1_compress per point, the cells put into the specs' order
             and byte-reversed with numpy.  The Montgomery product per cell value that leaving the blst_fr form also needs has no
             host entry point and is NOT counted: the figure flatters the route;
  * t_new    kzg_blobs_to_cells_and_proofs_bytes, all three outputs.
Both legs are timed at the same level: the C entry points through ctypes on contiguous arrays built beforehand.  For
information: kzg_cells_and_proofs_fk20 alone on coefficients decoded beforehand, kzg_commit_batch alone,
kzg_blobs_to_commitments_bytes alone.
GPU; medians of KZG_PERF_REPS calls (default 20) after a warm-up round.  The process pins itself to KZG_PERF_HOST_CPUS CPUs
(default 16) before anything starts a thread.  Writes JSON lines to profiles/r12_blob_bytes.jsonl (or the path given) and prints
them; KZG_PERF_REP tags the lines of one repetition of the script.  KZG_PERF_NEW_ONLY=1 runs the new call alone a few times and
writes nothing: the run a kernel trace is taken of."""
import json
import os
import random
import sys
import time

HOST_CPUS = int(os.environ.get("KZG_PERF_HOST_CPUS", "16"))
if HOST_CPUS > 0:  # before numpy or the library can start a thread: a pool made at import would keep the whole machine's mask
    os.sched_setaffinity(0, sorted(os.sched_getaffinity(0))[:HOST_CPUS])

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kzg_poly_commit_exploration_amd as K  # noqa: E402

REPS = int(os.environ.get("KZG_PERF_REPS", "20"))
REP = int(os.environ.get("KZG_PERF_REP", "0"))
NEW_ONLY = os.environ.get("KZG_PERF_NEW_ONLY", "0") == "1"
SECRET = bytes(range(32))
R = K.R_MODULUS
C = K.C


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


def brp_perm(bits):
    return np.array([int(format(i, "0%db" % bits)[::-1], 2) if bits else 0 for i in range(1 << bits)], dtype=np.int64)


def legs(lib, eng, B, n, log_n, log_l, rnd):
    lg = n.bit_length() - 1
    N, M, l = 1 << log_n, 1 << (log_n - log_l), 1 << log_l
    P = K._ptr
    blobs = np.frombuffer(b"".join(rnd.randrange(R).to_bytes(32, "big") for _ in range(B * n)), dtype=np.uint8).reshape(B, n, 32)
    blobs = np.ascontiguousarray(blobs)
    vals = np.zeros((B, n, 4), dtype=np.uint64)
    nat = np.zeros((B, n, 4), dtype=np.uint64)
    coeffs = np.zeros((B, n, 4), dtype=np.uint64)
    coms = np.zeros((B, 18), dtype=np.uint64)
    cells = np.zeros((B, N, 4), dtype=np.uint64)
    proofs = np.zeros((B, M, 18), dtype=np.uint64)
    r_coms = np.zeros((B, 48), dtype=np.uint8)
    r_proofs = np.zeros((B, M, 48), dtype=np.uint8)
    perm, cm, lm = brp_perm(lg), brp_perm(log_n - log_l), brp_perm(log_l)
    bad = C.c_size_t(0)
    lib.kzg_g1_compress.argtypes = [C.c_void_p, C.c_void_p]

    def route():
        assert lib.kzg_fr_from_bytes_batch(eng._h, P(blobs), B * n, P(vals), C.byref(bad)) == 0
        np.take(vals, perm, axis=1, out=nat)
        for b in range(B):
            assert lib.kzg_ntt(eng._h, nat[b].ctypes.data, n, 1, coeffs[b].ctypes.data) == 0
        assert lib.kzg_commit_batch(eng._h, P(coeffs), n, B, n, P(coms)) == 0
        assert lib.kzg_cells_and_proofs_fk20(eng._h, P(coeffs), n, B, n, log_n, log_l, P(cells), P(proofs)) == 0
        src, dst = coms.ctypes.data, r_coms.ctypes.data
        for b in range(B):
            lib.kzg_g1_compress(src + 144 * b, dst + 48 * b)
        ordered = np.ascontiguousarray(proofs[:, cm])
        src, dst = ordered.ctypes.data, r_proofs.ctypes.data
        for j in range(B * M):
            lib.kzg_g1_compress(src + 144 * j, dst + 48 * j)
        v = cells.reshape(B, M, l, 4)[:, cm][:, :, lm]
        return np.ascontiguousarray(v.view(np.uint8)[..., ::-1])  # (the Montgomery product is not counted)

    n_coms = np.zeros((B, 48), dtype=np.uint8)
    n_cells = np.zeros((B, N * 32), dtype=np.uint8)
    n_proofs = np.zeros((B, M * 48), dtype=np.uint8)

    def new():
        assert lib.kzg_blobs_to_cells_and_proofs_bytes(eng._h, P(blobs), n, B, n, log_n, log_l, K.KZG_ORDER_BIT_REVERSED, P(n_coms),
                                                       P(n_cells), P(n_proofs)) == 0

    def fk20_alone():
        assert lib.kzg_cells_and_proofs_fk20(eng._h, P(coeffs), n, B, n, log_n, log_l, P(cells), P(proofs)) == 0

    def commit_alone():
        assert lib.kzg_commit_batch(eng._h, P(coeffs), n, B, n, P(coms)) == 0

    def new_commit_alone():
        assert lib.kzg_blobs_to_commitments_bytes(eng._h, P(blobs), n, B, n, K.KZG_ORDER_BIT_REVERSED, P(n_coms)) == 0

    def check():
        route()
        new()
        assert np.array_equal(r_coms, n_coms) and np.array_equal(r_proofs.reshape(B, -1), n_proofs)

    return route, new, fk20_alone, commit_alone, new_commit_alone, check


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r12_blob_bytes.jsonl")
    lib = K.load_library()
    pinned = len(os.sched_getaffinity(0))
    recs = []
    n, log_n, log_l = 4096, 13, 6
    eng = K.SetupArtifactsGenerator(SECRET).take(n)
    try:
        eng.fk20_prepare(n, log_l)
        for B in (64, 1):
            route, new, fk20_alone, commit_alone, new_commit_alone, check = legs(lib, eng, B, n, log_n, log_l, random.Random(B))
            if NEW_ONLY:
                for _ in range(5):
                    new()
                continue
            check()
            t_route, t_new = alternate([route, new], REPS)
            t_fk20, t_commit, t_new_commit = alternate([fk20_alone, commit_alone, new_commit_alone], REPS)
            rec = {"what": "blobs_to_cells_and_proofs_bytes", "blobs": B, "n": n, "log_domain": log_n, "log_cell": log_l,
                   "order": "bit_reversed", "srs": n, "t_route_ms": round(1e3 * t_route, 3), "t_new_ms": round(1e3 * t_new, 3),
                   "t_route_over_t_new": round(t_route / t_new, 3), "t_fk20_alone_ms": round(1e3 * t_fk20, 3),
                   "t_commit_batch_alone_ms": round(1e3 * t_commit, 3),
                   "t_blobs_to_commitments_bytes_ms": round(1e3 * t_new_commit, 3),
                   "rep": REP, "reps": REPS, "host_cpus_pinned": pinned}
            recs.append(rec)
            print(json.dumps(rec), flush=True)
    finally:
        eng.close()
    if not NEW_ONLY:  # only a run that finished writes: a failed one leaves an earlier file as it was
        with open(out_path, "a" if REP else "w") as f:
            for rec in recs:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
