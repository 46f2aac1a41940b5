"""Batch verification of circuit proofs against the only route there was before it: a loop of
kzg_circuit_verify_proof spread over 16 host threads.  Shape t = 3, e = 4, n = 256, 16 public inputs; M = 1 ... 4096 proofs of one
key (32 and 48 beside the powers of four, to place the crossover), built by repeating eight distinct blinded proofs of
tests/transcript_oracle.py (the verifiers do the same work for a repeated proof as for any other).  GPU.

Both routes run in turn KZG_PERF_REPS times (default 5) after one warm-up round, on the same inputs; every line holds min, median
and max.  The process pins itself to KZG_PERF_HOST_CPUS CPUs (default 16) before anything starts a thread, so the host loop and
the batch call's own host threads have that many cores whatever the box shows.  Also timed: kzg_circuit_proof_challenges over the
same 16 threads (what the per-proof route hashes: it compresses the key anew for every proof), and the test hook with caller
weights with and without caller challenges -- the difference of the two is the batch call's own hashing (the key compressed once,
one SHA-256 chain per proof on up to 16 threads).  Writes JSON lines to profiles/r34_circuit_verify_batch.jsonl (or the path
given) and prints them; the last line names the crossover, the least measured M from which the batch call's median stays below
the host loop's.

`--kernels [M]`: five batch calls at M proofs (default 4096) and nothing else, for a separate `rocprofv3 --kernel-trace --stats`
run: per call k_wire_g1 and k_wire_fr (the decoders), k_cvb_public, k_cvb_lin, k_cvb_scalars, k_vc_fr_sum's levels and
k_cvb_key_split (the scalars), one k_vc_ladder (stage 1: the proofs' points and the key's), one k_cvb_stage2 (stage 2) and the
k_vc_g1_sum levels."""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bigint_twin as BT  # noqa: E402
import blind_oracle as BO  # noqa: E402
import circuit_oracle as CO  # noqa: E402
import kzg_poly_commit_exploration_amd as K  # noqa: E402
import oracle_ctypes  # noqa: E402
import transcript_oracle as TR  # noqa: E402

REPS = int(os.environ.get("KZG_PERF_REPS", "5"))
MS = [int(x) for x in os.environ.get("KZG_PERF_MS", "1,16,32,48,64,256,1024,4096").split(",") if x]
HOST_CPUS = int(os.environ.get("KZG_PERF_HOST_CPUS", "16"))
THREADS = 16
N, T, LOG_EXT, N_PUBLIC, DISTINCT = 256, 3, 2, 16, 8
S = BT.fr_from_be_bytes(BT.BENCH_SECRET_BE)


def circuit():
    """a satisfied circuit whose public inputs sit in the first N_PUBLIC rows: the later rows' move into q_C"""
    c = CO.satisfied(8, T, 3400, True)
    for i in range(N_PUBLIC, N):
        c.q_const[i] = (c.q_const[i] + c.pi[i]) % CO.R
        c.pi[i] = 0
    assert CO.gate_rows(c) == [0] * N
    return c


def alternate(fns, reps):
    """per call [min, median, max] in seconds, the calls run in turn `reps` times after one warm-up round"""
    for fn in fns:
        fn()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ts[i].append(time.perf_counter() - t0)
    return [[float(np.min(t)), float(np.median(t)), float(np.max(t))] for t in ts]


def ms(triple):
    return [round(1e3 * x, 3) for x in triple]


def main():
    if HOST_CPUS > 0:
        os.sched_setaffinity(0, sorted(os.sched_getaffinity(0))[:HOST_CPUS])
    args = sys.argv[1:]
    kernels = "--kernels" in args
    if kernels:
        at = args.index("--kernels")
        m_kernels = int(args[at + 1]) if at + 1 < len(args) else 4096
        args = args[:at]
    out = args[0] if args else os.path.join(ROOT, "profiles", "r34_circuit_verify_batch.jsonl")
    oracle_ctypes.lib()
    c = circuit()
    ds = [TR.prove(oracle_ctypes, c, LOG_EXT, BO.Blinders.random(T, LOG_EXT, 3400 + i), S, n_public=N_PUBLIC) for i in range(DISTINCT)]
    key = [K.G1Point.uncompress(k) for k in ds[0]["key48"]]
    shifts = [K.Scalar(k) for k in c.ks]
    public = [K.Scalar(p) for p in ds[0]["public"]]
    assert len(public) == N_PUBLIC
    g1 = np.stack([oracle_ctypes.p1_generator()])
    g2 = np.stack([K.srs_g2_at(BT.BENCH_SECRET_BE, j) for j in range(3)])
    lib = K.load_library()
    eng = K.SetupArtifactsGenerator(BT.BENCH_SECRET_BE).take(64)
    pool = ThreadPoolExecutor(THREADS)
    recs = []

    def emit(rec):
        recs.append(rec)
        print(json.dumps(rec), flush=True)

    try:
        # the per-proof calls' arguments, made once per distinct proof: the loop is the C calls alone
        t, rows, ks, pub, n_public, _ = K._proof_statement(key, shifts, public, ds[0]["proof"])
        bufs = [np.frombuffer(d["proof"], dtype=np.uint8) for d in ds]
        oks = [K.C.c_int(0) for _ in range(THREADS)]
        chs = [np.zeros((5, 4), dtype=np.uint64) for _ in range(THREADS)]

        def verify_part(th, m):
            for k in range(th, m, THREADS):
                buf = bufs[k % DISTINCT]
                rc = lib.kzg_circuit_verify_proof(K._ptr(rows), N, t, LOG_EXT, K._ptr(ks), K._ptr(pub), n_public, K._ptr(buf), buf.shape[0],
                                                  K._ptr(g1), 144, K._ptr(g2), 288, K.C.byref(oks[th]))
                assert rc == 0 and oks[th].value == 1

        def hash_part(th, m):
            for k in range(th, m, THREADS):
                buf = bufs[k % DISTINCT]
                rc = lib.kzg_circuit_proof_challenges(K._ptr(rows), N, t, LOG_EXT, K._ptr(ks), K._ptr(pub), n_public, K._ptr(buf),
                                                      buf.shape[0], K._ptr(chs[th]))
                assert rc == 0

        for m in ([m_kernels] if kernels else MS):
            proofs = [ds[k % DISTINCT]["proof"] for k in range(m)]
            pubs = np.broadcast_to(pub, (m,) + pub.shape).copy()
            _, _, a = eng._circuit_verify_batch_args(key, N, LOG_EXT, shifts, pubs, proofs, g2, None, None)
            ok, bad = K.C.c_int(0), K.C.c_size_t(0)
            wts = K.scalars_to_limbs([(0x9E3779B97F4A7C15 * (k + 1)) % K.R_MODULUS for k in range(m)])
            chal = np.stack([np.stack([c.limbs() for c in K.circuit_proof_challenges(key, N, LOG_EXT, shifts, public, d["proof"])])
                             for d in ds])
            chals = np.ascontiguousarray(chal[[k % DISTINCT for k in range(m)]])
            out3 = np.zeros((3, 18), dtype=np.uint64)

            def hook_hashed():
                rc = lib.kzg_circuit_verify_proofs_lincomb(eng._h, *a, K._ptr(wts), K._ptr(out3), K.C.byref(ok), K.C.byref(bad))
                assert rc == 0 and ok.value == 1

            def hook_given():
                rc = lib.kzg_circuit_verify_proofs_lincomb_challenges(eng._h, *a, K._ptr(wts), K._ptr(chals), K._ptr(out3), K.C.byref(ok),
                                                                      K.C.byref(bad))
                assert rc == 0 and ok.value == 1

            def batch():
                rc = lib.kzg_circuit_verify_proofs_batch(eng._h, *a, K.C.byref(ok), K.C.byref(bad))
                assert rc == 0 and ok.value == 1

            def host_loop():
                list(pool.map(lambda th: verify_part(th, m), range(min(THREADS, m))))

            def hashing():
                list(pool.map(lambda th: hash_part(th, m), range(min(THREADS, m))))

            if kernels:
                for _ in range(5):
                    batch()
                continue
            t_batch, t_host, t_hash, t_hooked, t_given = alternate([batch, host_loop, hashing, hook_hashed, hook_given], REPS)
            emit({"what": "circuit_verify_proofs_batch", "measured": True, "n": N, "t": T, "e": 1 << LOG_EXT, "n_public": N_PUBLIC, "proofs": m,
                  "distinct_proofs": min(m, DISTINCT), "reps": REPS, "host_cpus_pinned": len(os.sched_getaffinity(0)),
                  "host_threads": min(THREADS, m), "batch_call_ms_min_med_max": ms(t_batch),
                  "verify_proof_loop_ms_min_med_max": ms(t_host), "proof_challenges_loop_ms_min_med_max": ms(t_hash),
                  "hook_hashed_ms_min_med_max": ms(t_hooked), "hook_given_challenges_ms_min_med_max": ms(t_given),
                  "batch_own_hashing_ms_by_difference_of_medians": round(1e3 * (t_hooked[1] - t_given[1]), 3),
                  "speedup_of_medians": round(t_host[1] / t_batch[1], 2)})
        if not kernels:
            ahead = [r["proofs"] for r in recs if r["speedup_of_medians"] > 1]
            behind = [r["proofs"] for r in recs if r["speedup_of_medians"] <= 1]
            first = min((p for p in ahead if all(b < p for b in behind)), default=None)
            emit({"what": "crossover", "measured": True, "batch_ahead_from_proofs": first,
                  "last_measured_behind": max(behind, default=None), "measured_at": [r["proofs"] for r in recs]})
    finally:
        pool.shutdown()
        eng.close()
        if not kernels:
            with open(out, "w") as f:
                for rec in recs:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
