"""GPU: every wrapper of include/kzg_mi355x.hpp on the device, byte for byte against the oracles.

tests/hpp/hpp_parity.cpp (built by build(), or here with g++ when the binary is missing) includes only the header.  This module
writes one file of input records from fixed seeds, runs the program ONCE in a child process, and compares every output record:
commitments and proofs with the known-secret oracle (tests/trapdoor_oracle.py), transforms with tests/ntt_oracle.py, cells with
tests/cells_oracle.py, circuit proofs, keys, quotients, evaluations and challenges with tests/transcript_oracle.py (which stands
on circuit_oracle / blind_oracle), point-set proofs with tests/open_sets_oracle.py, wire forms with tests/wire_oracle.py; where a
family has no scalar oracle for an output (the raw blst_p1 image of a point next to its compressed form, the bare circuit's plain
quotient) with the same call through the Python mirror on an engine of the same SRS, which the suite holds to the oracles.  All comparisons are exact.  Verifier wrappers must say true on the good
record and false on the altered one; every documented throw must arrive with its status."""
import os
import random
import struct
import subprocess
import time

import numpy as np
import pytest

import bigint_twin as BT
import blind_oracle as BO
import cells_oracle as CO
import circuit_proof_cases as CP  # satisfied circuits with the transcript oracle's proofs, computed once
import grand_product_oracle as GO
import kzg_poly_commit_exploration_amd as K
import ntt_oracle as NO
import open_sets_oracle as SO
import transcript_oracle as TR
import trapdoor_oracle as TO
import wire_oracle as WO

pytestmark = pytest.mark.gpu
R = NO.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "hpp", "hpp_parity")
S = BT.fr_from_be_bytes(BT.BENCH_SECRET_BE)
SRS = 80
# examples/perm_quotient is given 120 s by its test and takes 0.5 s of it on an MI355X; this program makes a few hundred small
# calls on four contexts and takes 1.0 s there, so the same bound is kept: a factor above 100 for a loaded machine
TIMEOUT = 120
CIRCUITS = {"circ_b": (8, 3, 2, True), "circ_p": (16, 2, 2, False)}


def _rand(n, seed):
    rnd = random.Random(77000 + seed)
    return [rnd.randrange(1, R) for _ in range(n)]


def _limbs(values):
    return GO.to_limbs(list(values)).tobytes() if len(values) else b""


def _be(values):
    return b"".join(WO.fr_be(v) for v in values)


def _raw(points):
    """the blst_p1 images of mirror points, as the program writes them"""
    return b"".join(np.ascontiguousarray(p.p1 if isinstance(p, K.G1Point) else p, dtype=np.uint64).tobytes() for p in points)


def _c48(raw):
    assert len(raw) % 144 == 0
    return b"".join(K.G1Point(np.frombuffer(raw[i:i + 144], dtype=np.uint64).copy()).compress() for i in range(0, len(raw), 144))


def _u64(v):
    return struct.pack("<Q", v)


def _records(data):
    out, at = {}, 0
    while at < len(data):
        (ln,) = struct.unpack_from("<Q", data, at)
        name = data[at + 8:at + 8 + ln].decode()
        at += 8 + ln
        (ln,) = struct.unpack_from("<Q", data, at)
        assert name not in out, "record %s written twice" % name
        out[name] = data[at + 8:at + 8 + ln]
        at += 8 + ln
    assert at == len(data)
    return out


def _quotient_by_roots(vals, zs):
    """the quotient of P by prod (X - z_i): one synthetic division per root, the remainders dropped"""
    cur = [v % R for v in vals]
    for z in zs:
        q, acc = [0] * (len(cur) - 1), 0
        for i in range(len(cur) - 1, 0, -1):
            acc = (acc * z + cur[i]) % R
            q[i - 1] = acc
        cur = q
    return cur


class Case:
    """the inputs (name -> bytes) and what every output record has to be: raw (exact bytes), c48 (the points' compressed
    encodings), status (Error::status; the text is checked against kzg_strerror's prefix where the library speaks)"""

    def __init__(self):
        self.inputs, self.raw, self.c48, self.status = {}, {}, {}, {}

    def flag(self, name, value):
        self.raw[name] = _u64(1 if value else 0)


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE):
        lib = os.path.join(ROOT, "kzg_poly_commit_exploration_amd")
        subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), EXE + ".cpp", "-L" + lib, "-lkzg_mi355x",
                        "-Wl,-rpath,$ORIGIN/../../kzg_poly_commit_exploration_amd", "-o", EXE], check=True)
    return EXE


def _inputs_and_expectations(e, oracle, tmp):
    c = Case()
    I, W, W48 = c.inputs, c.raw, c.c48
    c40, c3, c81, pts, v64 = _rand(40, 1), _rand(120, 2), _rand(81, 3), _rand(5, 4), _rand(64, 5)
    padded = c40[:31] + [0] * 9
    gamma, z_out = _rand(1, 6)[0], _rand(1, 7)[0]
    w64 = NO.domain_root(6)
    z_in = pow(w64, 3, R)
    polys = [c3[0:40], c3[40:80], c3[80:120]]
    sc = K.Scalar
    I.update(secret=BT.BENCH_SECRET_BE, cache_path=os.path.join(tmp, "srs.cache").encode(), c40=_limbs(c40), c16=_limbs(c40[:16]),
             c40_top9_zero=_limbs(padded), c3x40=_limbs(c3), c81=_limbs(c81), pts=_limbs(pts), v64=_limbs(v64), gamma=_limbs([gamma]),
             z_out=_limbs([z_out]), z_in3=_limbs([z_in]))
    commit48 = lambda vals: TO.commitment(oracle, vals, S)
    ok = lambda name: c.status.__setitem__(name, K.KZG_OK)

    # ---- SetupArtifacts ----
    srs = oracle.srs_g1(SRS, BT.BENCH_SECRET_BE)
    srs48 = [oracle.p1_compress(p) for p in srs]
    W["srs.len"], W["srs16.len"], W["srs_io.len"], W["srs_io.multi.len"] = _u64(80), _u64(16), _u64(16), _u64(16)
    W["srs.read_0_1"], W["srs.read_3_13"], W["srs.read_79_1"] = _raw(e.srs_read(0, 1)), _raw(e.srs_read(3, 13)), _raw(e.srs_read(79, 1))
    W48["srs.read_0_1"], W48["srs.read_3_13"], W48["srs.read_79_1"] = srs48[0], b"".join(srs48[3:16]), srs48[79]
    for j in range(3):
        W["g2.%d" % j] = np.ascontiguousarray(K.srs_g2_at(BT.BENCH_SECRET_BE, j), dtype=np.uint64).tobytes()
    W["srs16.first0"], W["srs16.first5"] = _raw(e.srs_read(0, 16)), _raw(e.srs_read(5, 16))
    W48["srs16.first5"] = b"".join(srs48[5:21])
    for way in ("load", "load_compressed", "load_file"):
        W["srs_io." + way] = W["srs16.first5"]
    W48["srs_io.multi.commit"] = TO.g1_scalar(oracle, TO.commitment_scalar(c40[:16], S) * pow(S, 5, R))
    W["srs.max_batch"], W["srs.max_batch_back"] = _u64(3), _u64(1)

    # ---- Polynomial, Evaluation, batches ----
    W["try_from.full.len"], W["try_from.full.degree"] = _u64(40), _u64(39)
    W["try_from.padded.coefficients"], W["try_from.padded.degree"] = _limbs(padded[:31]), _u64(30)
    W["try_from.zeros.len"], W["try_from.empty.len"], W["try_from.empty.degree"] = _u64(1), _u64(0), _u64(0)
    l40 = GO.to_limbs(c40)
    y0 = TO.poly_eval(c40, pts[0])
    cm, pf = e.commit_limbs(l40), e.open_limbs(l40, sc(pts[0]), sc(y0))
    W["p40.commit"], W48["p40.commit"], W["p40.commit48"] = _raw([cm]), commit48(c40), commit48(c40)
    W["p40.eval"] = _limbs([y0])
    W["p40.proof"], W48["p40.proof"] = _raw([pf]), TO.proof(oracle, c40, pts[0], S)
    W48["p40.add"] = TO.g1_scalar(oracle, TO.commitment_scalar(c40, S) + TO.proof_scalar(c40, pts[0], S))
    c.flag("p40.verify", True), c.flag("p40.verify_wrong_value", False), c.flag("p40.verify_swapped", False)
    c.flag("p40.commit_is_infinity", False), c.flag("scalar.ops", True)
    W["const.proof"] = bytes(144)
    c.flag("const.proof_is_infinity", True), c.flag("const.verify", True)
    c.status["const.false_claim"] = K.KZG_ERR_CONSTANT_POLY
    c.status["false_claim"] = K.KZG_ERR_REMAINDER
    c.status["too_long"] = K.KZG_ERR_DEGREE_TOO_HIGH
    W48["batch.commit"] = b"".join(commit48(p) for p in polys)
    W["batch.commit"] = _raw([e.commit_limbs(GO.to_limbs(p)) for p in polys])
    W48["batch.open"] = b"".join(TO.proof(oracle, p, z, S) for p, z in zip(polys, pts))
    W48["batch.open_one_wrong.0"], W48["batch.open_one_wrong.2"] = W48["batch.open"][:48], W48["batch.open"][96:]
    W["batch.open_one_wrong.statuses"] = struct.pack("<3i", K.KZG_OK, K.KZG_ERR_REMAINDER, K.KZG_OK)

    # ---- Domain ----
    W["domain.root6"], W["domain.root0"] = _limbs([w64]), _limbs([1])
    for n in (1, 2, 64):
        W["domain.ntt.%d" % n], W["domain.intt.%d" % n] = _limbs(NO.ntt(v64[:n])), _limbs(NO.intt(v64[:n]))
    p64 = NO.intt(v64)
    W48["domain.commit"] = commit48(p64)
    W48["domain.proof_outside"], W48["domain.proof_inside"] = TO.proof(oracle, p64, z_out, S), TO.proof(oracle, p64, z_in, S)
    W["domain.commit"] = _raw([e.commit_evaluations_limbs(GO.to_limbs(v64))])
    c.status["domain.false_claim"] = K.KZG_ERR_REMAINDER

    # ---- Evaluations, combined openings, point sets ----
    for k in (1, 4, 5):
        name, zs = "pts%d" % k, pts[:k]
        ys = [TO.poly_eval(c40, z) for z in zs]
        W[name + ".results"] = _limbs(ys)
        W48[name + ".proof"] = TO.multiproof(oracle, c40, zs, S)
        W[name + ".proof"] = _raw([e.open_points_limbs(l40, [sc(z) for z in zs], [sc(y) for y in ys])])
        W[name + ".quotient"] = _limbs(_quotient_by_roots(c40, zs))
        assert len(W[name + ".quotient"]) == 32 * (40 - k)
        assert TO.poly_eval(_quotient_by_roots(c40, zs), S) == TO.multiproof_scalar(c40, zs, S)
        c.flag(name + ".verify", True), c.flag(name + ".verify_wrong_value", False)
        c.status[name + ".false_claim"] = K.KZG_ERR_REMAINDER
    ys, proof = e.open_combined_limbs([GO.to_limbs(p) for p in polys], sc(pts[0]), sc(gamma))
    assert [y.v for y in ys] == [TO.poly_eval(p, pts[0]) for p in polys]
    W["combined.results"], W["combined.proof"] = _limbs([y.v for y in ys]), _raw([proof])
    combined = [sum(pow(gamma, i, R) * p[j] for i, p in enumerate(polys)) % R for j in range(40)]
    W48["combined.proof"] = TO.proof(oracle, combined, pts[0], S)
    c.flag("combined.verify", True), c.flag("combined.verify_wrong_value", False)
    for name, ps, set_of, sets in (("sets_a", polys, [0, 1, 0], [[pts[0]], [pts[0], pts[1]]]),
                                   ("sets_b", polys[:2], [1, 0], [[pts[0], pts[1], pts[2]], [pts[3]]])):
        ys, proof = e.open_sets_limbs([GO.to_limbs(p) for p in ps], set_of, [[sc(z) for z in s] for s in sets], sc(gamma))
        for i, row in enumerate(ys):
            assert [y.v for y in row] == [TO.poly_eval(ps[i], z) for z in sets[set_of[i]]]
            W["%s.results.%d" % (name, i)] = _limbs([y.v for y in row])
        W[name + ".proof"] = _raw([proof])
        W48[name + ".proof"] = TO.g1_scalar(oracle, SO.proof_scalar(ps, set_of, sets, gamma, S))
        W[name + ".set_len"] = struct.pack("<%dI" % len(sets), *[len(s) for s in sets])
        W[name + ".flat_points"] = _limbs([z for s in sets for z in s])
        c.flag(name + ".verify", True), c.flag(name + ".verify_wrong_value", False)

    # ---- Cells ----
    for K_, t_ in ((6, 2), (6, 0), (6, 6)):
        name = "cells.%d_%d" % (K_, t_)
        cells, proofs = e.cells_and_proofs_limbs(l40, K_, t_)
        W[name + ".values"], W[name + ".proofs"] = _limbs(CO.cells(c40, K_, t_)), _raw(proofs)
        assert cells.tobytes() == W[name + ".values"]
        W48[name + ".proofs"] = b"".join(TO.multiproof(oracle, c40, CO.cell_points(K_, t_, j), S) for j in range(64 >> t_))
        cells, proofs = e.cells_and_proofs_from_evaluations_limbs(GO.to_limbs(v64[:32]), K_, t_)
        W[name + ".ev_values"], W[name + ".ev_proofs"] = _limbs(CO.cells(NO.intt(v64[:32]), K_, t_)), _raw(proofs)
        W48[name + ".ev_proofs"] = b"".join(TO.multiproof(oracle, NO.intt(v64[:32]), CO.cell_points(K_, t_, j), S) for j in range(64 >> t_))
    c.status["cells.3_4"] = c.status["cells.3_4.ev"] = K.KZG_ERR_INVALID_ARG
    for name, vals, first, count in (("cellq.full", c40, 0, 16), ("cellq.part", c40, 5, 3), ("cellq.padded", padded[:31], 0, 16)):
        W[name + ".count"] = _u64(count)
        for j in range(count):
            q = CO.stride_quotient(vals, 4, CO.cell_root(6, 2, first + j))
            assert len(q) == len(vals) - 4
            W["%s.%d" % (name, j)] = _limbs(q)
    ragged = [polys[0][:33], polys[1][:17], polys[2][:5]]
    W["fk20.count"] = _u64(3)
    for b, vals in enumerate(ragged):
        cells, proofs = e.cells_and_proofs_limbs(GO.to_limbs(vals), 6, 2)
        for side in ("fk20.", "fk20.of."):
            W["%svalues.%d" % (side, b)], W["%sproofs.%d" % (side, b)] = _limbs(CO.cells(vals, 6, 2)), _raw(proofs)
        W48["fk20.proofs.%d" % b] = b"".join(TO.multiproof(oracle, vals, CO.cell_points(6, 2, j), S) for j in range(16))
    idx, ids = [0, 1, 1, 0, 1], [3, 0, 15, 7, 7]
    rows = [CO.cells(ragged[b], 6, 2)[4 * j:4 * j + 4] for b, j in zip(idx, ids)]
    proofs48 = b"".join(TO.multiproof(oracle, ragged[b], CO.cell_points(6, 2, j), S) for b, j in zip(idx, ids))
    ids_brp, rows_brp = WO.cells_to_spec(ids, rows, 6, 2)
    wrong = [list(r) for r in rows]
    wrong[3][2] = (wrong[3][2] + 1) % R
    I.update({"vcells.ids_brp": struct.pack("<5I", *ids_brp), "vcells.commitments48": commit48(ragged[0]) + commit48(ragged[1]),
              "vcells.proofs48": proofs48, "vcells.cells_be": b"".join(_be(r) for r in rows),
              "vcells.cells_be_brp": b"".join(_be(r) for r in rows_brp), "vcells.cells_be_wrong": b"".join(_be(r) for r in wrong),
              "vcells.cells_be_brp_wrong": b"".join(_be(r) for r in WO.cells_to_spec(ids, wrong, 6, 2)[1])})
    assert ids_brp != ids
    for name, value in (("verify", True), ("verify_wrong_value", False), ("verify_empty", True), ("bytes.natural", True),
                        ("bytes.brp", True), ("bytes.natural_wrong_value", False), ("bytes.brp_wrong_value", False),
                        ("bytes.brp_as_natural", False)):
        c.flag("vcells." + name, value)
    c.status["vcells.short_g2"] = c.status["vcells.bytes.short_g2"] = K.KZG_ERR_INVALID_ARG

    # ---- Wire ----
    widx, wz = [0, 1, 1], pts[:3]
    wy = [TO.poly_eval(polys[b], z) for b, z in zip(widx, wz)]
    I.update({"wire.open.idx": struct.pack("<3I", *widx), "wire.open.commitments48": commit48(polys[0]) + commit48(polys[1]),
              "wire.open.zs_be": _be(wz), "wire.open.ys_be": _be(wy), "wire.open.ys_be_wrong": _be(wy[:2] + [(wy[2] + 1) % R]),
              "wire.open.proofs48": b"".join(TO.proof(oracle, polys[b], z, S) for b, z in zip(widx, wz))})
    c.flag("wire.openings", True), c.flag("wire.openings_wrong_value", False), c.flag("wire.openings_swapped", False)
    blobs = [v64[0:8], v64[8:16]]
    bcoef = [NO.intt(b) for b in blobs]
    bproofs = [TO.proof(oracle, p, z, S) for p, z in zip(bcoef, pts)]
    I.update({"wire.blobs.blobs_be": b"".join(_be(b) for b in blobs), "wire.blobs.blobs_be_brp": b"".join(_be(WO.blob_to_spec(b)) for b in blobs),
              "wire.blobs.commitments48": b"".join(commit48(p) for p in bcoef), "wire.blobs.zs_be": _be(pts[:2]),
              "wire.blobs.proofs48": b"".join(bproofs), "wire.blobs.proofs48_swapped": bproofs[1] + bproofs[0]})
    for name, value in (("blobs", True), ("blobs_with_ys", True), ("blobs_brp", True), ("blobs_wrong_proof", False)):
        c.flag("wire." + name, value)
    W["wire.blobs.ys_be"] = W["wire.blobs_brp.ys_be"] = _be([TO.poly_eval(p, z) for p, z in zip(bcoef, pts)])
    g2 = np.stack([K.srs_g2_at(BT.BENCH_SECRET_BE, j) for j in range(3)])
    try:  # batch = 0 through the mirror, on the same library: whatever it answers, the header has to answer the same
        valid, _ = e.verify_blobs_batch_bytes(b"", 8, b"", b"", b"", g2[:2])
        ok("wire.blobs_empty")
        c.flag("wire.blobs_empty.valid", valid)
    except K.KzgError as ex:
        c.status["wire.blobs_empty"] = ex.status
    W["wire.blobs_empty.ys_len"] = _u64(0)
    good48 = commit48(polys[0]) + bytes([0xC0]) + bytes(47) + commit48(polys[1])
    torsion = TO.torsion_points()
    bad48 = commit48(polys[0]) + WO.plus_torsion(commit48(polys[1]), torsion[11]) + commit48(polys[2])
    I.update({"wire.points48": good48, "wire.points48_torsion": bad48, "wire.fr_be": _be(v64[:3]), "wire.fr_be_bad": _be(v64[:2]) + WO.fr_be_raw(R)})
    W["wire.uncompress"] = W["wire.uncompress_subgroup"] = e.g1_uncompress_batch(good48, True).tobytes()
    W["wire.uncompress_torsion_unchecked"] = e.g1_uncompress_batch(bad48, False).tobytes()
    c.status["wire.uncompress_off_subgroup"] = c.status["wire.fr_not_below_r"] = c.status["wire.fr_ragged"] = K.KZG_ERR_INVALID_ARG
    ok("wire.uncompress_empty"), ok("wire.fr_empty")
    W["wire.uncompress_empty.len"] = W["wire.fr_empty.len"] = _u64(0)
    W["wire.fr"] = _limbs(v64[:3])

    # ---- Circuit ----
    for name, (n, t, log_ext, blinded) in CIRCUITS.items():
        e_ = 1 << log_ext
        bl, d = CP.case(oracle, n, t, log_ext, True, blinded)
        cc = d["c"]
        flat = lambda cols: _limbs([v for col in cols for v in col])
        put = lambda field, data: I.__setitem__(name + "." + field, data)
        put("q_lin", flat(cc.q_lin)), put("q_mul", _limbs(cc.q_mul)), put("q_const", _limbs(cc.q_const)), put("sigmas", flat(cc.sigmas))
        put("shifts", _limbs(cc.ks)), put("wires", flat(cc.wires)), put("z", _limbs(d["z"])), put("pi", _limbs(cc.pi))
        put("public", _limbs(d["public"])), put("blinders", _limbs(bl.flat()))
        for ch in ("alpha", "beta", "gamma", "zeta", "v"):
            put(ch, _limbs([d[ch]]))
        f = TR.split(d["proof"], t, log_ext)
        qlen = (e_ - 1) * n + (t + 3 if blinded else 0)
        T = list(d["T"])
        assert not any(T[qlen:])
        T = _limbs((T + [0] * qlen)[:qlen])
        W[name + ".bare.key_len"] = _u64(0)
        c.status[name + ".bare.prove"] = K.KZG_ERR_INVALID_ARG
        plainT = T
        circ = CP.create(e, cc, log_ext)
        try:
            shifts = [sc(k) for k in cc.ks]
            ch = [sc(d[x]) for x in ("alpha", "beta", "gamma", "zeta", "v")]
            wires, zz, pi = CP.limbs(cc.wires, n), GO.to_limbs(d["z"]), GO.to_limbs(cc.pi)
            W[name + ".key"] = _raw(circ.key)
            if blinded:  # the bare circuit's plain quotient of the same witness: through the mirror
                plainT = circ.quotient(wires, zz, ch[0], ch[1], ch[2], public_inputs=pi, want_commitments=False)[0].tobytes()
            else:
                evals, r = circ.linearise(wires, zz, np.frombuffer(T, dtype=np.uint64).reshape(-1, 4), ch[0], ch[1], ch[2], ch[3], public_inputs=pi)
                want_r = list(BO.linearisation(cc, d["coefs"], d["T"], log_ext, bl, d["alpha"], d["beta"], d["gamma"], d["zeta"]))
                assert not any(want_r[n:])
                W[name + ".linearise.r"] = _limbs((want_r + [0] * n)[:n])
                assert np.ascontiguousarray(r).tobytes() == W[name + ".linearise.r"], "the mirror's r differs from blind_oracle's"
        finally:
            circ.close()
        W[name + ".bare.quotient"] = plainT
        W48[name + ".key"] = b"".join(d["key48"])
        W[name + ".n"], W[name + ".t"], W[name + ".proof_size"] = _u64(n), _u64(t), _u64(TR.proof_size(t, log_ext))
        W[name + ".blinders_len"] = _u64(2 * t + 3 + e_ - 2)
        W[name + ".quotient"] = W[name + ".quotient_no_commitments"] = T
        W48[name + ".wire_commitments"], W48[name + ".z_commitment"], W48[name + ".t_commitments"], W48[name + ".w"] = \
            f["wires"], f["z"], f["chunks"], f["w"]
        abar, sbar, zw = d["evals"]
        W[name + ".evals"] = _limbs(list(abar) + list(sbar) + [zw])
        assert _be(list(abar) + list(sbar) + [zw]) == f["evals"]
        c.status[name + ".open_sizes"] = c.status[name + ".verify_sizes"] = c.status[name + ".verify_proof_short"] = K.KZG_ERR_INVALID_ARG
        if not blinded:
            W[name + ".quotient_zero_gate"] = T
            W[name + ".linearise.evals"] = W[name + ".open_device.evals"] = W[name + ".evals"]
            W48[name + ".open_device.proof"] = f["w"]
            for field in ("wires", "z", "pi"):
                c.status["%s.open_sizes.%s" % (name, field)] = K.KZG_ERR_INVALID_ARG
            W[name + ".column_len"], W[name + ".column_coset_len"] = _u64(n), _u64(e_ * n)
            W[name + ".column_sigma0"] = _limbs(cc.sigmas[0])
            c.status[name + ".open_device.resident_as_z"] = K.KZG_ERR_REMAINDER
        for flag, value in (("verify", True), ("verify_alpha_beta_swapped", False), ("verify_wrong_value", False), ("verify_proof", True),
                            ("verify_proof_flipped", False), ("move_ctor.handle", True), ("move_assign.handle", True)):
            c.flag("%s.%s" % (name, flag), value)
        W[name + ".proof"] = W[name + ".move_ctor.proof"] = W[name + ".move_assign.proof"] = d["proof"]
        W[name + ".challenges"] = _limbs([d[x] for x in ("beta", "gamma", "alpha", "zeta", "v")])
    W["done"] = _u64(1)
    return c


@pytest.fixture(scope="module")
def run(exe, engines, oracle, tmp_path_factory):
    """(the case, the output records): the program runs once for the module"""
    tmp = str(tmp_path_factory.mktemp("hpp_parity"))
    case = _inputs_and_expectations(engines.bench_srs(SRS), oracle, tmp)
    src, dst = os.path.join(tmp, "in.rec"), os.path.join(tmp, "out.rec")
    with open(src, "wb") as f:
        for name, data in case.inputs.items():
            f.write(_u64(len(name)) + name.encode() + _u64(len(data)) + data)
    t0 = time.perf_counter()
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=TIMEOUT)
    seconds = time.perf_counter() - t0
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    with open(dst, "rb") as f:
        got = _records(f.read())
    print("hpp_parity: %d input records, %d output records, %.2f s" % (len(case.inputs), len(got), seconds))
    return case, got


def test_every_record_is_expected_and_present(run):
    case, got = run
    want = set(case.raw) | set(case.c48)
    for name in case.status:
        want |= {name + ".status", name + ".what"}
    assert set(got) == want, {"missing": sorted(want - set(got)), "unexpected": sorted(set(got) - want)}


def test_outputs_equal_the_oracles_byte_for_byte(run):
    case, got = run
    wrong = [name for name, data in case.raw.items() if got.get(name) != data]
    wrong += [name + " (compressed)" for name, data in case.c48.items() if name not in got or _c48(got[name]) != data]
    assert not wrong, wrong


def test_every_documented_throw_arrives_with_its_status_and_the_librarys_text(run, engines):
    case, got = run
    e = engines.bench_srs(SRS)
    own = ("short_g2", "open_sizes", "verify_sizes", "bare.prove", "fr_ragged")  # the header's own Error, before any library call
    for name, status in case.status.items():
        (st,) = struct.unpack("<q", got[name + ".status"])
        what = got[name + ".what"].decode()
        assert st == status, (name, st, status, what)
        if status != K.KZG_OK and not any(tag in name for tag in own):
            assert what.startswith(e._lib.kzg_strerror(status).decode()), (name, what)
        if any(tag in name for tag in own):
            assert what and not what.startswith(e._lib.kzg_strerror(status).decode()), (name, what)
    assert "too high" in got["too_long.what"].decode()
