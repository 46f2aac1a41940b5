"""kzg_circuit_lookup_prove_device (DESIGN.md sections 4.26 and 5.0y) against kzg_circuit_prove_device, plain, on the SAME circuit
handle -- the parent commit's capability: a proof of the arithmetic and the permutation alone, the table ignored -- one device, one
process, warmed, five alternated repetitions (KZG_PERF_REPS) with their min-max, at n = 2^KZG_PERF_LOG (default 20), t = 3, c = 3,
e = 4, resident wires, 16 public inputs, a host clock around synchronous calls.
The witness is tests/perf_circuit.py's (equal wires in a row, a cyclic permutation); q_K selects the first half of the rows, the table
holds their tuples and, in its second half, the zero tuple (n / 2 duplicate rows: multiplicities n / 2 + 1 at one row, 1 and 0).
Before anything is timed both proofs are checked with their verifiers.
`--kernels`: a few lookup proofs and nothing else, for a separate `rocprofv3 --kernel-trace --stats` run (the spans of k_lk_fold and
k_lk_constraints); `--kernel-stats FILE` adds the two kernels' rows of that run's kernel_stats.csv to the output with the bytes each
moves.
GPU.  Writes JSON lines to profiles/r31_circuit_lookup.jsonl (or the path given) and prints them."""
import csv
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import kzg_poly_commit_exploration_amd as K  # noqa: E402
import perf_circuit as PC  # noqa: E402

REPS = max(int(os.environ.get("KZG_PERF_REPS", "5")), 3)
LOG_N = int(os.environ.get("KZG_PERF_LOG", "20"))
R = K.R_MODULUS
T, LOG_EXT, C_TAB, N_PUBLIC = PC.T, PC.LOG_EXT, 3, 16


def kernel_rows(path, n, N):
    """the two kernels' rows of a rocprofv3 kernel_stats.csv, with the bytes a launch moves (32 per value read or written)"""
    moved = {"k_lk_fold": 32 * n * (2 * C_TAB + 1 + 2), "k_lk_constraints": 32 * N * (2 * C_TAB + 1 + 1 + 1 + 2 + 1)}
    out = []
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            for name, nbytes in moved.items():
                if name in row.get("Name", ""):
                    avg_us = float(row["AverageNs"]) / 1e3
                    out.append({"what": name, "measured": True, "source": "rocprofv3 --kernel-trace --stats", "calls": int(row["Calls"]),
                                "avg_us": round(avg_us, 2), "min_us": round(float(row["MinNs"]) / 1e3, 2),
                                "max_us": round(float(row["MaxNs"]) / 1e3, 2), "bytes_moved": nbytes,
                                "gb_per_s": round(nbytes / avg_us / 1e3, 1)})
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    kernels_only = "--kernels" in sys.argv
    stats_csv = None
    if "--kernel-stats" in sys.argv:
        stats_csv = sys.argv[sys.argv.index("--kernel-stats") + 1]
        args = [a for a in args if a != stats_csv]
    out = args[0] if args else os.path.join(ROOT, "profiles", "r31_circuit_lookup.jsonl")
    n, e = 1 << LOG_N, 1 << LOG_EXT
    eng = K.SetupArtifactsGenerator(PC.SECRET).take(n)
    rng = np.random.default_rng(31)
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    d_w = None
    try:
        row, wires, sigmas, shifts = PC.cyclic_argument(eng, n, rng)
        q_lin, q_mul, pi = np.stack([PC.values(rng, n) for _ in range(T)]), PC.values(rng, n), PC.values(rng, n)
        pi[N_PUBLIC:] = 0
        f, qs, qm, p = PC.ints(row), [PC.ints(c) for c in q_lin], PC.ints(q_mul), PC.ints(pi)
        q_const = PC.limbs([(-((qs[0][i] + qs[1][i] + qs[2][i]) * f[i] + qm[i] * f[i] % R * PC.RINV % R * f[i]) % R * PC.RINV - p[i]) % R
                            for i in range(n)])
        del f, qs, qm, p
        q_k = np.zeros((n, 4), dtype=np.uint64)
        q_k[:n // 2] = K.Scalar(1).limbs()
        col = row.copy()
        col[n // 2:] = 0  # the zero tuple
        table = np.stack([col] * C_TAB)
        circ = eng.circuit_create_lookup(q_lin, q_mul, q_const, sigmas, shifts, LOG_EXT, table, q_k, want_key=True)
        d_w = eng.dev_alloc(wires.nbytes)
        eng.dev_upload(d_w, np.ascontiguousarray(wires))
        pub_rows = np.ascontiguousarray(pi[:N_PUBLIC])

        def prove_lookup():
            return circ.lookup_prove_device(d_w, pub_rows)

        def prove_plain():
            return circ.prove_device(d_w, pub_rows, None)

        if kernels_only:
            for _ in range(4):
                prove_lookup()
            return
        g1, g2 = eng.srs_read(0, 1), np.stack([K.srs_g2_at(PC.SECRET, j) for j in range(3)])
        public = [K.Scalar.from_limbs(x) for x in pub_rows]
        assert K.circuit_lookup_verify_proof(circ.key, n, LOG_EXT, C_TAB, shifts, public, prove_lookup(), g1, g2)
        assert K.circuit_verify_proof(circ.key[:2 * T + 2], n, LOG_EXT, shifts, public, prove_plain(), g1, g2)
        emit({"what": "proofs_verify", "measured": True, "log_n": LOG_N, "t": T, "c": C_TAB, "log_ext": LOG_EXT, "n_public": N_PUBLIC})
        prove_lookup(), prove_plain()  # warm
        ts = {"lookup": [], "plain": []}
        for _ in range(REPS):  # alternated
            ts["lookup"].append(PC.timed(prove_lookup))
            ts["plain"].append(PC.timed(prove_plain))
        base = {"measured": True, "log_n": LOG_N, "t": T, "c": C_TAB, "log_ext": LOG_EXT, "reps": REPS, "n_public": N_PUBLIC}
        emit(dict(base, what="circuit_lookup_prove_device", proof_bytes=K.circuit_lookup_proof_size(T, LOG_EXT, C_TAB), **PC.stats(ts["lookup"])))
        emit(dict(base, what="circuit_prove_device_plain_same_handle", proof_bytes=K.circuit_proof_size(T, LOG_EXT), **PC.stats(ts["plain"])))
        circ.close()
        if stats_csv:
            for line in kernel_rows(stats_csv, n, n * e):
                emit(dict(line, log_n=LOG_N, c=C_TAB))
    finally:
        if d_w is not None:
            eng.dev_free(d_w)
        eng.close()
    if kernels_only:
        return
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
