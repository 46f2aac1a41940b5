"""The verifiers on wire bytes against today's route, legs alternated call by call on the same inputs,
at the DAS shape (16 384 cells of 128 commitments, log_domain 13, log_cell 6) and at 4096 openings (64 commitments, every
record at its own point):
  * t_old          the existing call on inputs that are decoded already;
  * t_host_decode  producing those inputs from the wire bytes with today's public API: kzg_g1_uncompress per point, on 1 and
                   on 16 host threads, plus the byte reversal of the scalars with numpy.  The 16-thread figure is taken with a
                   Python thread pool whose workers call through ctypes point by point: the interpreter lock bounds it, so
                   every line also carries the one-thread time divided by 16, what a native pool could reach at best.  The
                   Montgomery product per scalar that the ABI's blst_fr form also needs has no host entry point and is NOT
                   counted;
  * t_new          the _bytes call on the wire bytes.
Both device legs are timed at the same level: the C entry points through ctypes on contiguous arrays built beforehand, so
no wrapper's argument handling is inside either figure.
GPU; medians of KZG_PERF_REPS calls (default 20) after a warm-up round.  The process pins itself to KZG_PERF_HOST_CPUS CPUs
(default 16) before anything starts a thread.  Writes JSON lines to profiles/r11_wire_bytes.jsonl (or the path given) and
prints them; KZG_PERF_REP tags the lines of one repetition of the script."""
import json
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kzg_poly_commit_exploration_amd as K  # noqa: E402
import oracle_ctypes as O  # noqa: E402

REPS = int(os.environ.get("KZG_PERF_REPS", "20"))
HOST_CPUS = int(os.environ.get("KZG_PERF_HOST_CPUS", "16"))
REP = int(os.environ.get("KZG_PERF_REP", "0"))
SECRET = bytes(range(32))
R = K.R_MODULUS


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


def be_bytes(limbs):
    """blst_fr rows -> their big-endian strings, (count, 32) uint8"""
    ints = K.limbs_to_scalars(limbs)
    return np.frombuffer(b"".join(v.to_bytes(32, "big") for v in ints), dtype=np.uint8).reshape(-1, 32)


def compress(rows):
    return np.frombuffer(b"".join(O.p1_compress(r) for r in rows), dtype=np.uint8).reshape(-1, 48)


def host_decoder(lib, points48, scalars_be, threads, pool):
    """today's route from the wire bytes to the ABI's inputs (see the module's note on what is not counted)"""
    n = points48.shape[0]
    out = np.zeros((n, 18), dtype=np.uint64)
    src, dst = points48.ctypes.data, out.ctypes.data

    def part(lo, hi):
        for i in range(lo, hi):
            lib.kzg_g1_uncompress(K.C.c_char_p(src + 48 * i), K.C.c_void_p(dst + 144 * i))

    def run():
        if threads == 1:
            part(0, n)
        else:
            step = (n + threads - 1) // threads
            list(pool.map(lambda t: part(t * step, min(n, (t + 1) * step)), range(threads)))
        np.ascontiguousarray(scalars_be[:, ::-1]).view(np.uint64)  # little-endian limbs (not yet Montgomery)
        return out

    return run


def main():
    if HOST_CPUS > 0:
        os.sched_setaffinity(0, sorted(os.sched_getaffinity(0))[:HOST_CPUS])
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r11_wire_bytes.jsonl")
    lib = K.load_library()
    lib.kzg_g1_uncompress.argtypes = [K.C.c_char_p, K.C.c_void_p]
    pool = ThreadPoolExecutor(16)
    pinned = len(os.sched_getaffinity(0))
    recs = []

    def emit(rec):
        rec.update({"rep": REP, "reps": REPS, "host_cpus_pinned": pinned})
        recs.append(rec)
        print(json.dumps(rec), flush=True)

    n, log_n, log_l, B = 4096, 13, 6, 128
    M, l = 1 << (log_n - log_l), 1 << log_l
    g2 = [K.srs_g2_at(SECRET, i) for i in range(l + 1)]
    eng = K.SetupArtifactsGenerator(SECRET).take(n)
    try:
        # ---- cells at the DAS shape
        base = np.ascontiguousarray(O.bench_coefficients(n), dtype=np.uint64).reshape(n, 4)
        c = np.repeat(base[None], B, axis=0)
        c[:, 0, 0] = np.arange(B, dtype=np.uint64) + 1
        cells, proofs = eng.cells_and_proofs_fk20(c, log_n, log_l)
        coms = np.stack([eng.commit_limbs(c[b]).p1 for b in range(B)])
        vals = cells.reshape(B, M, l, 4)
        prf = np.stack([np.stack([p.p1 for p in proofs[b]]) for b in range(B)])
        k = 16384
        rnd = random.Random(k)
        rows = [(rnd.randrange(B), rnd.randrange(M)) for _ in range(k)]
        idx = np.array([r[0] for r in rows], dtype=np.uint32)
        ids = np.array([r[1] for r in rows], dtype=np.uint32)
        rv = np.ascontiguousarray(vals[idx, ids])
        rp = np.ascontiguousarray(prf[idx, ids])
        all_be = be_bytes(vals.reshape(-1, 4)).reshape(B, M, l, 32)
        all_prf48 = compress(prf.reshape(-1, 18)).reshape(B, M, 48)
        coms48 = compress(coms)
        cells_be = np.ascontiguousarray(all_be[idx, ids])
        prf48 = np.ascontiguousarray(all_prf48[idx, ids])
        points48 = np.ascontiguousarray(np.concatenate([prf48, coms48]))

        g2a = np.ascontiguousarray(np.stack(g2))
        ok = K.C.c_int(0)
        P = K._ptr

        def old():
            rc = lib.kzg_verify_cells_batch(eng._h, P(coms), B, P(idx), P(ids), P(rv), P(rp), k, log_n, log_l, P(g2a), 288,
                                            K.C.byref(ok))
            assert rc == 0 and ok.value == 1

        def new():
            rc = lib.kzg_verify_cells_batch_bytes(eng._h, P(coms48), B, P(idx), P(ids), P(cells_be), P(prf48), k, log_n, log_l, 0,
                                                  P(g2a), 288, K.C.byref(ok))
            assert rc == 0 and ok.value == 1

        dec1 = host_decoder(lib, points48, cells_be.reshape(-1, 32), 1, pool)
        dec16 = host_decoder(lib, points48, cells_be.reshape(-1, 32), 16, pool)
        assert np.array_equal(dec16(), np.concatenate([rp, coms])) and np.array_equal(dec1(), dec16())
        t_old, t_new, t_d16 = alternate([old, new, dec16], REPS)
        t_d1 = alternate([dec1], max(3, REPS // 5))[0]
        emit({"what": "verify_cells_batch_bytes", "cells": k, "commitments": B, "log_domain": log_n, "log_cell": log_l,
              "points_decoded": int(points48.shape[0]), "scalars": k * l,
              "t_old_ms": round(1e3 * t_old, 3), "t_new_ms": round(1e3 * t_new, 3),
              "t_host_decode_1_thread_ms": round(1e3 * t_d1, 3), "t_host_decode_16_threads_ms": round(1e3 * t_d16, 3),
              "t_host_decode_1_thread_over_16_ms": round(1e3 * t_d1 / 16, 3),
              "t_new_minus_t_old_ms": round(1e3 * (t_new - t_old), 3),
              "t_old_plus_host_decode_16_ms": round(1e3 * (t_old + t_d16), 3),
              "t_old_plus_ideal_host_decode_ms": round(1e3 * (t_old + t_d1 / 16), 3)})
        # ---- openings: polynomials a + b X, whose quotient is b at every point
        ko, Bo = 4096, 64
        ab = [(rnd.randrange(R), rnd.randrange(R)) for _ in range(Bo)]
        limbs = [K.scalars_to_limbs(list(p)) for p in ab]
        ocoms = np.stack([eng.commit_limbs(x).p1 for x in limbs])
        oprfs = np.stack([eng.open_limbs(x, K.Scalar(3), K.Scalar((a + 3 * b) % R)).p1 for x, (a, b) in zip(limbs, ab)])
        oidx = np.array([rnd.randrange(Bo) for _ in range(ko)], dtype=np.uint32)
        zs = [rnd.randrange(R) for _ in range(ko)]
        ys = [(ab[b][0] + ab[b][1] * z) % R for b, z in zip(oidx, zs)]
        zl, yl = K.scalars_to_limbs(zs), K.scalars_to_limbs(ys)
        rp_o = np.ascontiguousarray(oprfs[oidx])
        zs_be = np.frombuffer(b"".join(z.to_bytes(32, "big") for z in zs), dtype=np.uint8).reshape(-1, 32)
        ys_be = np.frombuffer(b"".join(y.to_bytes(32, "big") for y in ys), dtype=np.uint8).reshape(-1, 32)
        ocoms48 = compress(ocoms)
        oprf48 = np.ascontiguousarray(compress(oprfs)[oidx])
        opoints48 = np.ascontiguousarray(np.concatenate([oprf48, ocoms48]))
        oscalars = np.ascontiguousarray(np.concatenate([zs_be, ys_be]))

        def oold():
            rc = lib.kzg_verify_openings_batch(eng._h, P(ocoms), Bo, P(oidx), P(zl), P(yl), P(rp_o), ko, P(g2a), 288, K.C.byref(ok))
            assert rc == 0 and ok.value == 1

        def onew():
            rc = lib.kzg_verify_openings_batch_bytes(eng._h, P(ocoms48), Bo, P(oidx), P(zs_be), P(ys_be), P(oprf48), ko, P(g2a), 288,
                                                     K.C.byref(ok))
            assert rc == 0 and ok.value == 1

        odec1 = host_decoder(lib, opoints48, oscalars, 1, pool)
        odec16 = host_decoder(lib, opoints48, oscalars, 16, pool)
        assert np.array_equal(odec16(), np.concatenate([rp_o, ocoms]))
        t_old, t_new, t_d16 = alternate([oold, onew, odec16], REPS)
        t_d1 = alternate([odec1], max(3, REPS // 5))[0]
        emit({"what": "verify_openings_batch_bytes", "records": ko, "commitments": Bo, "points": "distinct",
              "points_decoded": int(opoints48.shape[0]), "scalars": 2 * ko,
              "t_old_ms": round(1e3 * t_old, 3), "t_new_ms": round(1e3 * t_new, 3),
              "t_host_decode_1_thread_ms": round(1e3 * t_d1, 3), "t_host_decode_16_threads_ms": round(1e3 * t_d16, 3),
              "t_host_decode_1_thread_over_16_ms": round(1e3 * t_d1 / 16, 3),
              "t_new_minus_t_old_ms": round(1e3 * (t_new - t_old), 3),
              "t_old_plus_host_decode_16_ms": round(1e3 * (t_old + t_d16), 3),
              "t_old_plus_ideal_host_decode_ms": round(1e3 * (t_old + t_d1 / 16), 3)})
    finally:
        eng.close()
        pool.shutdown()
        with open(out_path, "a" if REP else "w") as f:
            for rec in recs:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
