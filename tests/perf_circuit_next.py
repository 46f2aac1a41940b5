"""kzg_circuit_custom_next_prove_device (DESIGN.md sections 4.28 and 5.0aa) against kzg_circuit_custom_prove_device on a TWIN custom
circuit whose terms have the same exponents all at the current row -- [[5,0,0],[1,1,1]] against p = [[3,0,0],[1,1,0]] and
p' = [[2,0,0],[0,0,1]]: the same number of products per point, so that what differs is the second, cache-served load in the gate
kernel, one more evaluation pass, one more column at zeta w and 32 more proof bytes per wire of R -- one device, one process, warmed,
alternated repetitions (KZG_PERF_REPS, at least 3) with their min-max, at n = 2^KZG_PERF_LOG (19: e = 8 and N <= 2^22), t = 3, e = 8,
resident wires, 16 public inputs, a host clock around synchronous calls.  The two verifiers are timed on the host (the next-row
one has a third set and with it one more pairing).
The witness is tests/perf_circuit.py's (equal wires in a row, a cyclic permutation); the twin has qx_1 = -qx_0 f^2, the next-row
circuit qx_1[i] = -qx_0[i] f[i] f[i+1] (i + 1 mod n), so that the two terms cancel on H and both statements hold on the same wires.
Before anything is timed both proofs are checked with their verifiers.
`--kernels`: four proofs of each kind and nothing else, for a separate `rocprofv3 --kernel-trace --stats` run (k_cgn_gate against
k_cg_gate); `--kernel-stats FILE` adds the two kernels' rows of that run's kernel_stats.csv to the output.
GPU.  Writes JSON lines to profiles/r33_circuit_next.jsonl (or the path given) and prints them."""
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import kzg_poly_commit_exploration_amd as K  # noqa: E402
import perf_circuit as PC  # noqa: E402

REPS = max(int(os.environ.get("KZG_PERF_REPS", "5")), 3)
LOG_N = int(os.environ.get("KZG_PERF_LOG", "19"))
R = K.R_MODULUS
T, LOG_EXT, N_PUBLIC = PC.T, 3, 16
TWIN = [[5, 0, 0], [1, 1, 1]]
EXPS, EXPS_NEXT = [[3, 0, 0], [1, 1, 0]], [[2, 0, 0], [0, 0, 1]]


def kernel_rows(path):
    """the two gate kernels' rows of a rocprofv3 kernel_stats.csv"""
    out = []
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name", "")
            for k in ("k_cgn_gate", "k_cg_gate"):
                if k in name:
                    out.append({"what": k, "measured": True, "source": "rocprofv3 --kernel-trace --stats", "calls": int(row["Calls"]),
                                "avg_us": round(float(row["AverageNs"]) / 1e3, 2), "min_us": round(float(row["MinNs"]) / 1e3, 2),
                                "max_us": round(float(row["MaxNs"]) / 1e3, 2)})
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    kernels_only = "--kernels" in sys.argv
    stats_csv = None
    if "--kernel-stats" in sys.argv:
        stats_csv = sys.argv[sys.argv.index("--kernel-stats") + 1]
        args = [a for a in args if a != stats_csv]
    out = args[0] if args else os.path.join(ROOT, "profiles", "r33_circuit_next.jsonl")
    n = 1 << LOG_N
    eng = K.SetupArtifactsGenerator(PC.SECRET).take(n + T + 3)
    rng = np.random.default_rng(33)
    lines = []

    def emit(line):
        lines.append(line)
        print(json.dumps(line), flush=True)

    d_w = None
    try:
        row, wires, sigmas, shifts = PC.cyclic_argument(eng, n, rng)
        q_lin, q_mul, pi, qx0 = np.stack([PC.values(rng, n) for _ in range(T)]), PC.values(rng, n), PC.values(rng, n), PC.values(rng, n)
        pi[N_PUBLIC:] = 0
        f, qs, qm, p, x0 = PC.ints(row), [PC.ints(c) for c in q_lin], PC.ints(q_mul), PC.ints(pi), PC.ints(qx0)
        # images (x 2^256): a b RINV is the image of the product.  The base gate holds row by row
        q_const = PC.limbs([(-((qs[0][i] + qs[1][i] + qs[2][i]) * f[i] + qm[i] * f[i] % R * PC.RINV % R * f[i]) % R * PC.RINV - p[i]) % R
                            for i in range(n)])
        twin_qx1 = PC.limbs([(-(x0[i] * f[i] % R * PC.RINV % R * f[i] % R * PC.RINV)) % R for i in range(n)])
        next_qx1 = PC.limbs([(-(x0[i] * f[i] % R * PC.RINV % R * f[(i + 1) % n] % R * PC.RINV)) % R for i in range(n)])
        del f, qs, qm, p, x0
        twin = eng.circuit_create_custom(q_lin, q_mul, q_const, sigmas, shifts, LOG_EXT, np.stack([qx0, twin_qx1]), TWIN, want_key=True)
        circ = eng.circuit_create_custom_next(q_lin, q_mul, q_const, sigmas, shifts, LOG_EXT, np.stack([qx0, next_qx1]), EXPS, EXPS_NEXT,
                                              want_key=True)
        d_w = eng.dev_alloc(wires.nbytes)
        eng.dev_upload(d_w, np.ascontiguousarray(wires))
        pub_rows = np.ascontiguousarray(pi[:N_PUBLIC])
        runs = {"twin_custom": lambda: twin.custom_prove_device(d_w, pub_rows, None),
                "next_row": lambda: circ.custom_next_prove_device(d_w, pub_rows, None)}
        if kernels_only:
            for _ in range(4):
                for fn in runs.values():
                    fn()
            return
        g1, g2 = eng.srs_read(0, 2), np.stack([K.srs_g2_at(PC.SECRET, j) for j in range(3)])
        public = [K.Scalar.from_limbs(x) for x in pub_rows]
        proofs = {name: fn() for name, fn in runs.items()}
        verifiers = {"twin_custom": lambda: K.circuit_custom_verify_proof(twin.key, n, LOG_EXT, TWIN, shifts, public, proofs["twin_custom"], g1, g2),
                     "next_row": lambda: K.circuit_custom_next_verify_proof(circ.key, n, LOG_EXT, EXPS, EXPS_NEXT, shifts, public,
                                                                            proofs["next_row"], g1, g2)}
        for name, fn in verifiers.items():
            assert fn(), name
        emit({"what": "proofs_verify", "measured": True, "log_n": LOG_N, "t": T, "log_ext": LOG_EXT, "twin_exponents": TWIN,
              "exponents": EXPS, "exponents_next": EXPS_NEXT, "n_public": N_PUBLIC})
        for fn in runs.values():
            fn()  # warm
        ts, vs = {name: [] for name in runs}, {name: [] for name in runs}
        for _ in range(REPS):  # alternated
            for name, fn in runs.items():
                ts[name].append(PC.timed(fn))
            for name, fn in verifiers.items():
                t0 = time.perf_counter()
                fn()
                vs[name].append(time.perf_counter() - t0)
        base = {"measured": True, "log_n": LOG_N, "t": T, "log_ext": LOG_EXT, "reps": REPS, "n_public": N_PUBLIC}
        emit(dict(base, what="circuit_custom_prove_device_twin", exponents=TWIN, proof_bytes=len(proofs["twin_custom"]),
                  **PC.stats(ts["twin_custom"])))
        emit(dict(base, what="circuit_custom_next_prove_device", exponents=EXPS, exponents_next=EXPS_NEXT, rho=circ.rho,
                  proof_bytes=len(proofs["next_row"]), **PC.stats(ts["next_row"])))
        emit(dict(base, what="circuit_custom_verify_proof_twin_host", **PC.stats(vs["twin_custom"])))
        emit(dict(base, what="circuit_custom_next_verify_proof_host", **PC.stats(vs["next_row"])))
        twin.close()
        circ.close()
        if stats_csv:
            for line in kernel_rows(stats_csv):
                emit(dict(line, log_n=LOG_N))
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
