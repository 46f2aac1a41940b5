"""kzg_circuit_custom_prove_device, plain and blinded (DESIGN.md sections 4.27 and 5.0z), against kzg_circuit_prove_device, plain
and blinded, on the SAME circuit handle -- the parent commit's capability: a proof of the arithmetic gate and the permutation
alone, the custom terms ignored -- one device, one process, warmed, three alternated repetitions (KZG_PERF_REPS) with their min-max,
at n = 2^KZG_PERF_LOG, t = 3, e = 8, resident wires, 16 public inputs, two terms with the exponents [[5,0,0],[1,1,1]], a host clock
around synchronous calls.
KZG_PERF_LOG defaults to 19: d_max = 5 asks for e = 8, and N = e n may not pass 2^22, the library's largest domain, so n = 2^20
cannot be run in this shape.
The witness is tests/perf_circuit.py's (equal wires in a row, a cyclic permutation); qx_1 = -qx_0 f^2 on every row, so that the two
terms cancel on H (G' vanishes there, not as a polynomial) and both statements hold: the same handle serves both provers.
Before anything is timed the four proofs are checked with their verifiers.
`--kernels`: a few custom proofs and nothing else, for a separate `rocprofv3 --kernel-trace --stats` run (the span of k_cg_gate);
`--kernel-stats FILE` adds the kernel's row of that run's kernel_stats.csv to the output with the bytes it moves,
(wires used + g + 1) N 32, and that rate as a fraction of the streaming HBM rate.
GPU.  Writes JSON lines to profiles/r32_circuit_custom.jsonl (or the path given) and prints them."""
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

REPS = max(int(os.environ.get("KZG_PERF_REPS", "3")), 3)
LOG_N = int(os.environ.get("KZG_PERF_LOG", "19"))
R = K.R_MODULUS
T, LOG_EXT, N_PUBLIC = PC.T, 3, 16
EXPS = [[5, 0, 0], [1, 1, 1]]
HBM_STREAMING_TB_S = 6.29  # what a float4 copy streams on an MI355X (8.0 TB/s is the specification)


def kernel_rows(path, N):
    """the kernel's row of a rocprofv3 kernel_stats.csv, with the bytes a launch moves (32 per value read or written)"""
    wires_used = sum(1 for j in range(T) if any(row[j] for row in EXPS))
    nbytes = 32 * N * (wires_used + len(EXPS) + 1)
    out = []
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            if "k_cg_gate" in row.get("Name", ""):
                avg_us = float(row["AverageNs"]) / 1e3
                rate = nbytes / avg_us / 1e6  # TB/s
                out.append({"what": "k_cg_gate", "measured": True, "source": "rocprofv3 --kernel-trace --stats", "calls": int(row["Calls"]),
                            "avg_us": round(avg_us, 2), "min_us": round(float(row["MinNs"]) / 1e3, 2),
                            "max_us": round(float(row["MaxNs"]) / 1e3, 2), "bytes_moved": nbytes, "tb_per_s": round(rate, 3),
                            "fraction_of_streaming_hbm": round(rate / HBM_STREAMING_TB_S, 3)})
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    kernels_only = "--kernels" in sys.argv
    stats_csv = None
    if "--kernel-stats" in sys.argv:
        stats_csv = sys.argv[sys.argv.index("--kernel-stats") + 1]
        args = [a for a in args if a != stats_csv]
    out = args[0] if args else os.path.join(ROOT, "profiles", "r32_circuit_custom.jsonl")
    n, e = 1 << LOG_N, 1 << LOG_EXT
    eng = K.SetupArtifactsGenerator(PC.SECRET).take(n + T + 3)
    rng = np.random.default_rng(32)
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
        # images (x 2^256): a b RINV is the image of the product.  The base gate holds row by row, and qx_1 = -qx_0 f^2
        q_const = PC.limbs([(-((qs[0][i] + qs[1][i] + qs[2][i]) * f[i] + qm[i] * f[i] % R * PC.RINV % R * f[i]) % R * PC.RINV - p[i]) % R
                            for i in range(n)])
        qx1 = PC.limbs([(-(x0[i] * f[i] % R * PC.RINV % R * f[i] % R * PC.RINV)) % R for i in range(n)])
        del f, qs, qm, p, x0
        circ = eng.circuit_create_custom(q_lin, q_mul, q_const, sigmas, shifts, LOG_EXT, np.stack([qx0, qx1]), EXPS, want_key=True)
        d_w = eng.dev_alloc(wires.nbytes)
        eng.dev_upload(d_w, np.ascontiguousarray(wires))
        pub_rows = np.ascontiguousarray(pi[:N_PUBLIC])
        bl = circ.blinders()
        K.circuit_custom_blinded_sizes(n, T, LOG_EXT, 5)  # (the blinded rule holds at this shape)
        runs = {"custom_plain": lambda: circ.custom_prove_device(d_w, pub_rows, None),
                "custom_blinded": lambda: circ.custom_prove_device(d_w, pub_rows, bl),
                "base_plain": lambda: circ.prove_device(d_w, pub_rows, None),
                "base_blinded": lambda: circ.prove_device(d_w, pub_rows, bl)}
        if kernels_only:
            for _ in range(4):
                runs["custom_plain"]()
            return
        g1, g2 = eng.srs_read(0, 1), np.stack([K.srs_g2_at(PC.SECRET, j) for j in range(3)])
        public = [K.Scalar.from_limbs(x) for x in pub_rows]
        for name, fn in runs.items():
            if name.startswith("custom"):
                assert K.circuit_custom_verify_proof(circ.key, n, LOG_EXT, EXPS, shifts, public, fn(), g1, g2), name
            else:
                assert K.circuit_verify_proof(circ.key[:2 * T + 2], n, LOG_EXT, shifts, public, fn(), g1, g2), name
        emit({"what": "proofs_verify", "measured": True, "log_n": LOG_N, "t": T, "log_ext": LOG_EXT, "exponents": EXPS, "n_public": N_PUBLIC})
        for fn in runs.values():
            fn()  # warm
        ts = {name: [] for name in runs}
        for _ in range(REPS):  # alternated
            for name, fn in runs.items():
                ts[name].append(PC.timed(fn))
        base = {"measured": True, "log_n": LOG_N, "t": T, "log_ext": LOG_EXT, "exponents": EXPS, "reps": REPS, "n_public": N_PUBLIC,
                "proof_bytes": K.circuit_proof_size(T, LOG_EXT)}
        what = {"custom_plain": "circuit_custom_prove_device", "custom_blinded": "circuit_custom_prove_device_blinded",
                "base_plain": "circuit_prove_device_same_handle", "base_blinded": "circuit_prove_device_blinded_same_handle"}
        for name in runs:
            emit(dict(base, what=what[name], **PC.stats(ts[name])))
        circ.close()
        if stats_csv:
            for line in kernel_rows(stats_csv, n * e):
                emit(dict(line, log_n=LOG_N, exponents=EXPS))
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
