"""GPU: the host-side pass loops around the prover kernels, at shapes where each loop takes a second turn.

* pq_extend walks its columns in chunks of min(64, budget / (4 N 32)) and the host form of kzg_coset_extend in rounds of
  budget / (N 32) columns.  Batches of 65, 128 and 129 columns pass the cap of 64 with the default budget of 2^30 bytes;
  KZG_PQ_WS_KB=256 (read when a context is created) brings the budget down so that the composite calls -- the permutation
  quotient, kzg_circuit_create, the circuit's quotient, its linearisation and opening -- walk their 7 to 16 columns in chunks of
  1, 2 and 4.  Without the knob the same calls return the same bytes.
* a range-split multi-device context exchanges a batch's partial sums in pieces of 64 (multi.hip).
* the barycentric evaluation stages at most 2^22 values per pass: 1025 polynomials of 4096 values take two.

Every value is compared limb for limb with the big-integer oracles (tests/perm_quotient_oracle.py, circuit_oracle.py,
linearise_oracle.py, ntt_oracle.py), every point with the known-secret shortcut of tests/trapdoor_oracle.py.  The coset extension
is linear, so the wide batches are column (j mod 7) of seven random columns times (j + 1): every column differs from every other,
a chunk written to another chunk's place shows, and the oracle extends seven columns.  Device outputs lie in a guard-banded arena
(tests/device_arena.py), which names the region, column and row of a difference."""
import numpy as np
import pytest

import bigint_twin as BT
import device_arena as DA
import grand_product_oracle as GO
import kzg_poly_commit_exploration_amd as K
import linearise_oracle as LO
import ntt_oracle as NO
import open_sets_oracle as SO
import perm_quotient_oracle as PQ
import test_circuit_open_gpu as TCO  # its memoised circuits, quotients and linearisations
import test_device_bounds_gpu as TDB  # _resident: every column a circuit hands out
import test_perm_quotient_gpu as TPQ  # its memoised permutation arguments
import trapdoor_oracle as TO
import wire_oracle as W

pytestmark = pytest.mark.gpu
R = PQ.R
S = BT.fr_from_be_bytes(BT.BENCH_SECRET_BE)
ALPHA, BETA, GAMMA, ZETA, V = TCO.ALPHA, TCO.BETA, TCO.GAMMA, TCO.ZETA, TCO.V
SRS = 2048
KNOB = "KZG_PQ_WS_KB"
WIDE = 129  # the widest batch: two chunks of 64 and one column more
_CACHE = {}  # references computed once, shared and left unchanged


def _memo(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _knob_engine(monkeypatch, srs=SRS):
    monkeypatch.setenv(KNOB, "256")
    return K.SetupArtifactsGenerator(BT.BENCH_SECRET_BE).take(srs) if srs else K.Engine(0)


def _plain_engine(monkeypatch, engines, srs=SRS):
    monkeypatch.delenv(KNOB, raising=False)
    return engines.bench_srs(srs)


def _strided(cols, stride):
    """(batch, len, 4) -> (batch, stride, 4); the rows past len hold words no value has"""
    out = np.full((cols.shape[0], stride, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    out[:, :cols.shape[1]] = cols
    return out


# ---- wide batches of the coset extension -------------------------------------------------------------------------------------------
def _wide(length, log_N, form, cols=WIDE):
    """(inputs (cols, length, 4), values on the coset (cols, N, 4)): column j is base column j mod 7 times j + 1.  VALUES: length
    values over the domain; COEFFS: length coefficients"""
    def make():
        base = [TPQ._rand(length, 300 + j) for j in range(7)]
        coefs = [NO.intt(b) for b in base] if form == K.KZG_EXTEND_VALUES else base
        ext = [PQ.coset_extend(c, log_N) for c in coefs]
        inp = np.stack([GO.to_limbs([(j + 1) * v % R for v in base[j % 7]]) for j in range(cols)])
        want = np.stack([GO.to_limbs([(j + 1) * v % R for v in ext[j % 7]]) for j in range(cols)])
        assert len({row.tobytes() for row in want}) == cols  # every column differs from every other
        return inp, want
    return _memo(("wide", length, log_N, form, cols), make)


def _extend_both_ways(e, length, log_N, batch, form, stride, inp, want, seed):
    N = 1 << log_N
    with DA.Arena(e, seed=seed) as ar:
        d_in = ar.region(length, batch, stride, name="in", data=inp[:batch])
        d_out = ar.region(N, batch, name="out")
        ar.upload()
        e.coset_extend_device(d_in.ptr, length, batch, log_N, d_out.ptr, form=form, stride=stride)
        ar.check(outputs={d_out: want[:batch]})
    got = e.coset_extend_limbs(_strided(inp[:batch], stride), log_N, form=form, n=length)
    differ = [j for j in range(batch) if not np.array_equal(got[j], want[j])]
    assert not differ, "host form: columns %s differ from the oracle" % differ[:8]
    return got


@pytest.fixture(scope="module")
def eng():
    e = K.Engine(0)  # the extension needs no SRS
    yield e
    e.close()


@pytest.mark.parametrize("batch", [65, 128, 129])
@pytest.mark.parametrize("length,log_N", [(4, 3), (1 << 11, 12)], ids=["dft", "ntt"])
def test_more_columns_than_one_chunk(eng, length, log_N, batch):
    """64 columns per chunk: 64 + 1, 64 + 64, 64 + 64 + 1.  N = 8 takes one batched DFT per chunk (and a 2D copy where stride is
    not len), N = 2^12 one launch_ntt per column"""
    for form in (K.KZG_EXTEND_VALUES, K.KZG_EXTEND_COEFFS):
        inp, want = _wide(length, log_N, form)
        for stride in (length, length + 5):
            _extend_both_ways(eng, length, log_N, batch, form, stride, inp, want, seed=batch + stride)


# ---- KZG_PQ_WS_KB=256: chunks of 2, 4 and 1 column, rounds of 8 and 1 ------------------------------------------------------------------
@pytest.mark.parametrize("length,log_N,cols", [(256, 10, 19), (1000, 10, 19), (2048, 13, 3)], ids=["values", "coeffs", "ntt"])
def test_extension_in_rounds_and_chunks(engines, monkeypatch, length, log_N, cols):
    """N = 2^10: 19 columns from host pointers in rounds of 8, 8, 3 with chunks of 2 inside, 19 columns on the device in chunks of
    2; N = 2^13: one column per round and chunk, launch_ntt per column"""
    form = K.KZG_EXTEND_COEFFS if length == 1000 else K.KZG_EXTEND_VALUES
    inp, want = _wide(length, log_N, form, cols)
    plain = _plain_engine(monkeypatch, engines)
    e = _knob_engine(monkeypatch, 0)
    try:
        for stride in (length, length + 5):
            got = _extend_both_ways(e, length, log_N, cols, form, stride, inp, want, seed=cols + stride)
            assert np.array_equal(got, plain.coset_extend_limbs(_strided(inp, stride), log_N, form=form, n=length))
    finally:
        e.close()


def _gate_term(n, N, T):
    """(G = Z_H Rc as coefficients, T + Rc): the caller's term that adds Rc to the quotient"""
    Rc = TPQ._rand(n, 80)
    gate = [((Rc[k - n] if n <= k < 2 * n else 0) - (Rc[k] if k < n else 0)) % R for k in range(2 * n)]
    full = list(T) + [0] * (N - n - len(T))
    return gate, [(a + (Rc[k] if k < n else 0)) % R for k, a in enumerate(full)]


@pytest.mark.parametrize("n,log_ext,t,seed", [(256, 2, 3, 70 + 256), (64, 3, 7, 77), (2048, 2, 3, 70 + 2048)])
def test_permutation_quotient_in_chunks(engines, oracle, monkeypatch, n, log_ext, t, seed):
    """2 t + 1 columns: 7 in chunks of 2 (N = 2^10), 15 in chunks of 4 (N = 2^9), 7 in chunks of 1 (N = 2^13)"""
    N = n << log_ext
    ks, wires, sigmas, z, T = TPQ._argument(NO.log2_exact(n), t, seed)
    gate, T1 = _memo(("gate", n, log_ext), lambda: _gate_term(n, N, T))
    gate_coset = GO.to_limbs(_memo(("gate-coset", n, log_ext), lambda: PQ.coset_extend(gate, NO.log2_exact(N))))
    args = (TPQ._limbs(wires, n + 3), TPQ._limbs(sigmas, n + 3), GO.to_limbs(z)) + tuple(TPQ._sc(ks)) + (log_ext,)
    plain = _plain_engine(monkeypatch, engines)
    e = _knob_engine(monkeypatch)
    try:
        for g, want in ((None, T), (gate_coset, T1)):
            coeffs, points = e.permutation_quotient(*args, gate=g, n=n)
            TPQ._check_composite(e, oracle, n, log_ext, want, coeffs, points)
            c0, p0 = plain.permutation_quotient(*args, gate=g, n=n)  # the default budget: byte for byte the same
            assert coeffs.tobytes() == c0.tobytes() and [p.p1.tobytes() for p in points] == [p.p1.tobytes() for p in p0]
    finally:
        e.close()


def _circuit_calls(e, oracle, n, t, log_ext, checked):
    """kzg_circuit_create with its key, the resident columns, the quotient with public inputs on host and device pointers, the
    linearisation and the opening on e -> every byte they returned.  checked: compare with the oracles"""
    N = n << log_ext
    c, z, T, coefs = TCO._case(n, t, True)
    r, evals, stack = TCO._lin(n, t, log_ext, True)
    want_t = TCO._t_limbs(T, n, log_ext)
    wires, zl, pi = TCO._limbs(c.wires, n + 5), GO.to_limbs(z), TCO._pi(c)
    circ = TCO._create(e, c, log_ext, want_key=True)
    try:
        resident = TDB._resident(e, circ, t)
        t_coeffs, t_points = circ.quotient(wires, zl, *TCO._ch()[:3], public_inputs=pi)
        with DA.Arena(e, seed=n + t) as ar:
            d_w = ar.region(n, t, n + 5, name="wires", data=TDB._lim(c.wires))
            d_t = ar.region(N - n, name="T")
            d_z = ar.region(n, name="z", data=zl)
            d_pi = ar.region(n, name="pi", data=pi)
            ar.upload()
            circ.quotient_device(d_w.ptr, d_z.ptr, *TCO._ch()[:3], d_t.ptr, d_public_inputs=d_pi.ptr, stride=n + 5)
            dev_evals, dev_proof = circ.open_device(d_w.ptr, d_z.ptr, d_t.ptr, *TCO._ch(), d_public_inputs=d_pi.ptr, stride=n + 5)
            ar.check(outputs={d_t: want_t})
        lin_evals, got_r = circ.linearise(wires, zl, t_coeffs, *TCO._ch()[:4], public_inputs=pi)
        got_evals, proof = circ.open(wires, zl, t_coeffs, *TCO._ch(), public_inputs=pi)
        if checked:
            key_cols, key_coefs = c.key_columns(), coefs[0]
            assert len(circ.key) == 2 * t + 2
            for j, point in enumerate(circ.key):  # q_lin[0..t), q_mul, q_const, sigma[0..t)
                assert point.compress() == TO.g1_scalar(oracle, PQ.horner(key_coefs[j], S)), j
            which = [K.KZG_CIRCUIT_COL_QLIN + j for j in range(t)] + [K.KZG_CIRCUIT_COL_QM, K.KZG_CIRCUIT_COL_QC] + \
                    [K.KZG_CIRCUIT_COL_SIGMA + j for j in range(t)]
            for j, w in enumerate(which):
                assert np.array_equal(resident[w, K.KZG_CIRCUIT_VALUES], GO.to_limbs(key_cols[j])), j
                assert np.array_equal(resident[w, K.KZG_CIRCUIT_COEFFS], GO.to_limbs(key_coefs[j])), j
                ext = _memo(("key-coset", n, t, log_ext, j), lambda: GO.to_limbs(PQ.coset_extend(key_coefs[j], NO.log2_exact(N))))
                assert np.array_equal(resident[w, K.KZG_CIRCUIT_COSET], ext), j
            l0 = _memo(("l0", n, log_ext), lambda: GO.to_limbs(PQ.coset_extend([pow(n, R - 2, R)] * n, NO.log2_exact(N))))
            assert np.array_equal(resident[K.KZG_CIRCUIT_COL_L0, K.KZG_CIRCUIT_COSET], l0)
            assert np.array_equal(t_coeffs, want_t)
            full = [v for ch in LO.chunks(T, n, log_ext) for v in ch]
            for k, point in enumerate(t_points):
                assert point.compress() == TO.g1_scalar(oracle, PQ.horner(full[k * n:(k + 1) * n], S)), k
            assert TCO._values(lin_evals) == evals and TCO._values(got_evals) == evals and TCO._values(dev_evals) == evals
            assert np.array_equal(got_r, GO.to_limbs(r))
            want_proof = TO.g1_scalar(oracle, SO.proof_scalar(stack[0], stack[1], stack[2], V, S))
            assert proof.compress() == want_proof and dev_proof.compress() == want_proof
        out = [p.p1.tobytes() for p in circ.key + t_points + [proof, dev_proof]]
        out += [resident[key].tobytes() for key in sorted(resident)]
        out += [t_coeffs.tobytes(), got_r.tobytes()]
        out += [x.limbs().tobytes() for ev in (lin_evals, got_evals, dev_evals) for x in ev[0] + ev[1] + [ev[2]]]
        return out
    finally:
        circ.close()


@pytest.mark.parametrize("n,t,log_ext", [(256, 3, 2), (64, 7, 3), (2048, 3, 2)])
def test_circuit_calls_in_chunks(engines, oracle, monkeypatch, n, t, log_ext):
    """kzg_circuit_create extends 2 t + 2 columns, the quotient t + 2: in chunks of 2, 4 and 1"""
    plain = _plain_engine(monkeypatch, engines)
    e = _knob_engine(monkeypatch)
    try:
        got = _circuit_calls(e, oracle, n, t, log_ext, True)
    finally:
        e.close()
    want = _circuit_calls(plain, oracle, n, t, log_ext, False)
    assert len(got) == len(want)
    assert [i for i, (a, b) in enumerate(zip(got, want)) if a != b] == []  # the default budget: byte for byte the same


# ---- the exchange of a batch's partial sums in pieces of 64 ----------------------------------------------------------------------------
def _batch_polys(count, n):
    """count polynomials of n coefficients, all different"""
    def make():
        polys = [TPQ._rand(n, 400 + b) for b in range(count)]
        assert len({tuple(p) for p in polys}) == count
        return polys, np.stack([GO.to_limbs(p) for p in polys])
    return _memo(("batch", count, n), make)


def _commitments(oracle, polys):
    return [_memo(("com", tuple(p)), lambda: TO.commitment(oracle, p, S)) for p in polys]


def test_exchange_over_rccl_in_pieces(oracle, monkeypatch):
    monkeypatch.setenv("KZG_MULTI_FORCE_RCCL", "1")
    polys, limbs = _batch_polys(WIDE, 16)
    want = _commitments(oracle, polys)
    e = K.Engine(devices=[0])
    try:
        e.srs_generate(BT.BENCH_SECRET_BE, 16)
        e.set_max_batch(4)
        for batch in (65, 128, 129):
            before = e.rccl_exchanges()
            got = [p.compress() for p in e.commit_batch_host(limbs[:batch])]
            differ = [b for b in range(batch) if got[b] != want[b]]
            assert not differ, "batch %d: commitments %s differ from [P(s)]G" % (batch, differ[:8])
            assert e.rccl_exchanges() - before == (batch + 63) // 64
    finally:
        e.close()


def test_exchange_on_the_host_with_empty_slices(oracle, monkeypatch):
    """three slices of 6, 5, 5 points and polynomials of 5 coefficients: the partial sums of slices 1 and 2 are the point at
    infinity, laid out device-major behind the 129 of slice 0"""
    monkeypatch.delenv("KZG_MULTI_FORCE_RCCL", raising=False)
    polys, limbs = _batch_polys(WIDE, 5)
    assert polys[64] != polys[0] and polys[128] != polys[0] and polys[128] != polys[64]
    want = _commitments(oracle, polys)
    e = K.Engine(devices=[0, 0, 0])
    try:
        e.srs_generate(BT.BENCH_SECRET_BE, 16)
        e.set_max_batch(4)
        got = [p.compress() for p in e.commit_batch_host(limbs)]
        differ = [b for b in range(WIDE) if got[b] != want[b]]
        assert not differ, "commitments %s differ from [P(s)]G" % differ[:8]
        # ... and with every slice at work: 16 coefficients
        polys16, limbs16 = _batch_polys(WIDE, 16)
        got = [p.compress() for p in e.commit_batch_host(limbs16)]
        assert got == _commitments(oracle, polys16)
    finally:
        e.close()


# ---- two passes of the barycentric evaluation -----------------------------------------------------------------------------------------
BARY_N, BARY_BATCH = 4096, 1025  # 1024 polynomials fill the 2^22 values of one pass


def _bary_case():
    """1025 polynomials in evaluation form -- eight cubics tiled over the first pass, a ninth at index 1024 -- one distinct point
    each, two of them in the domain, and the values by Horner"""
    def make():
        cubics = [TPQ._rand(4, 500 + j) for j in range(9)]
        of = [b % 8 for b in range(BARY_BATCH - 1)] + [8]
        base = np.stack([GO.to_limbs(NO.ntt(c + [0] * (BARY_N - 4))) for c in cubics])
        zs = list(TPQ._rand(BARY_BATCH, 510))
        w = NO.domain_root(12)
        zs[7], zs[1019] = pow(w, 5, R), pow(w, 4095, R)
        assert len(set(zs)) == BARY_BATCH
        ys = [PQ.horner(cubics[j], z) for j, z in zip(of, zs)]
        return cubics, of, base, zs, ys
    return _memo("bary", make)


def _bary_evals(stride):
    cubics, of, base, zs, ys = _bary_case()
    evals = np.full((BARY_BATCH, stride, 4), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)  # the gaps hold no value below r
    evals[:, :BARY_N] = base[of]
    return evals


@pytest.fixture(scope="module")
def bary_engine():
    e = K.SetupArtifactsGenerator(BT.BENCH_SECRET_BE).take(BARY_N)
    yield e
    e.close()


@pytest.mark.parametrize("stride", [BARY_N, BARY_N + 3])
def test_evaluation_in_two_passes(bary_engine, stride):
    e = bary_engine
    cubics, of, base, zs, ys = _bary_case()
    evals, zl = _bary_evals(stride), GO.to_limbs(zs)
    out = np.zeros((BARY_BATCH, 4), dtype=np.uint64)
    rc = e._lib.kzg_evaluate_evaluations_batch(e._h, evals.ctypes.data, BARY_N, BARY_BATCH, stride, zl.ctypes.data, out.ctypes.data)
    assert rc == K.KZG_OK, e._error(rc)
    want = GO.to_limbs(ys)
    differ = [b for b in range(BARY_BATCH) if not np.array_equal(out[b], want[b])]
    assert not differ, "values %s differ from Horner's" % differ[:8]


def _bary_records(oracle):
    def make():
        cubics, of, base, zs, ys = _bary_case()
        coms = [K.G1Point.uncompress(TO.commitment(oracle, c, S)) for c in cubics]
        proofs = [K.G1Point.uncompress(TO.proof(oracle, cubics[j], z, S)) for j, z in zip(of, zs)]
        g2 = np.stack([K.srs_g2_at(BT.BENCH_SECRET_BE, j) for j in range(2)])
        return [coms[j] for j in of], proofs, g2
    return _memo("bary-records", make)


def test_verification_of_evaluations_in_two_passes(bary_engine, oracle):
    """kzg_verify_evaluations_batch: the values stay on the device, the verifier reads value b at d_ys + 8 b words"""
    e = bary_engine
    cubics, of, base, zs, ys = _bary_case()
    coms, proofs, g2 = _bary_records(oracle)
    stride = BARY_N + 3
    evals, zl = _bary_evals(stride), GO.to_limbs(zs)
    com, prf = e._p1_rows(coms), e._p1_rows(proofs)
    out = np.zeros((BARY_BATCH, 4), dtype=np.uint64)
    ok = K.C.c_int(0)

    def run():
        rc = e._lib.kzg_verify_evaluations_batch(e._h, evals.ctypes.data, BARY_N, BARY_BATCH, stride, com.ctypes.data, zl.ctypes.data,
                                                 prf.ctypes.data, g2.ctypes.data, 288, out.ctypes.data, K.C.byref(ok))
        assert rc == K.KZG_OK, e._error(rc)
        return bool(ok.value)
    assert run()
    assert np.array_equal(out, GO.to_limbs(ys))
    # another value for record 1024: one evaluation of its polynomial changed, so what it opens to is no longer what the proof says
    evals[1024, 9] = GO.to_limbs([1 + GO.from_limbs(evals[1024, 9])[0]])[0]
    assert not run()
    assert np.array_equal(out[:1024], GO.to_limbs(ys[:1024])) and not np.array_equal(out[1024], GO.to_limbs(ys[1024:])[0])


def test_a_value_not_below_r_in_the_second_pass_is_named(bary_engine, oracle):
    """kzg_verify_blobs_batch_bytes: the device finds the value while it decodes pass 2; its index there is 0 x 4096 + 77"""
    e = bary_engine
    cubics, of, base, zs, ys = _bary_case()
    coms, proofs, g2 = _bary_records(oracle)
    blobs = np.stack([np.frombuffer(b"".join(W.fr_be(v) for v in GO.from_limbs(b)), dtype=np.uint8) for b in base])[of]
    blobs = blobs.reshape(BARY_BATCH * BARY_N, 32)
    coms48 = b"".join(p.compress() for p in coms)
    proofs48 = b"".join(p.compress() for p in proofs)
    zs_be = b"".join(W.fr_be(z) for z in zs)
    ok, ys_be = e.verify_blobs_batch_bytes(blobs, BARY_N, coms48, zs_be, proofs48, g2)
    assert ok and ys_be == b"".join(W.fr_be(y) for y in ys)
    blobs[1024 * BARY_N + 77] = np.frombuffer(W.fr_be_raw(R), dtype=np.uint8)
    with pytest.raises(K.KzgError) as ei:
        e.verify_blobs_batch_bytes(blobs, BARY_N, coms48, zs_be, proofs48, g2)
    assert ei.value.status == K.KZG_ERR_INVALID_ARG
    said = e._lib.kzg_last_error(e._h).decode()
    assert "polynomial 1024: value 77 is not below r" in said, said
