// hpp_parity.cpp -- every wrapper of include/kzg_mi355x.hpp run on the device; tests/test_hpp_parity_gpu.py writes the input
// records, runs this program ONCE (one process, one GPU initialisation) and compares every output record byte for byte with
// the oracles of tests/ (DESIGN.md section 4.2f).  It includes nothing of the project but the header under test and prints
// nothing a test has to parse.  Usage: hpp_parity <input file> <output file>.
// Record format, both files: u64 name length, name, u64 data length, data; scalars and points are blst's memory images.
// Build:  g++ -std=c++17 -Iinclude tests/hpp/hpp_parity.cpp -Lkzg_poly_commit_exploration_amd -lkzg_mi355x -o tests/hpp/hpp_parity
//
// wrapper                                          case (prefix of its output records)
// ------------------------------------------------ --------------------------------------------------------------------
// SetupArtifacts(int), generate, len, ctx          srs.* (80 points), srs16.* (first = 0 and first = 5)
// SetupArtifacts::read_g1, g2_at, set_max_batch    srs.read_*, g2.*, srs.max_batch
// SetupArtifacts::load, load_compressed, save,     srs_io.*: the 16 points read back after each way in
//   load_file, SetupArtifacts(vector<int>, bool)
// Scalar, G1Point::compress / is_infinity / add    scalar.ops, p40.commit48, p40.add, const.proof_is_infinity
// Polynomial::try_from, degree, coefficients       try_from.*
// Polynomial::commit, evaluate_at                  p40.commit, p40.eval
// commit_batch, open_batch                         batch.*
// Evaluation::generate_proof, verify_proof         p40.proof, p40.verify*, const.*, false_claim.*
// Domain::root, ntt, commit, generate_proof        domain.*
// Evaluations::at, generate_proof, quotient,       pts<k>.* for k = 1, 4, 5
//   verify_proof
// open_combined, verify_combined                   combined.*
// open_sets, verify_sets, SetsOpening::set_len,    sets_a.* (the shape of examples/open_sets.cpp), sets_b.* (a set of one
//   flat_points                                      point)
// Cells::of, of_evaluations                        cells.<log_domain>_<log_cell>.*
// Cells::quotients                                 cellq.*
// Cells::of_many_fk20, prepare_fk20                fk20.*
// Cells::verify_batch, verify_batch_bytes          vcells.*
// Wire::verify_openings, verify_blobs,             wire.*
//   g1_uncompress_batch, fr_from_bytes_batch
// Circuit: <c> = circ_b, blinded (8, 3, 2) with public inputs, and circ_p, plain (16, 2, 2)
//   Circuit(..., want_key = false), key             <c>.bare.key_len, <c>.bare.prove, <c>.bare.quotient
//   Circuit(...), key, n, t, handle                 <c>.key, <c>.n, <c>.t, <c>.move_ctor.handle
//   proof_size, blinders                            <c>.proof_size, <c>.blinders_len
//   commit_blinded (nb = 2 and nb = 3)              circ_b.wire_commitments, circ_b.z_commitment
//   quotient_blinded, open_blinded                  circ_b.quotient, .quotient_no_commitments, .t_commitments, .evals, .w, .open_sizes
//   quotient (public inputs, gate_coset, no commitments)  circ_p.quotient, .quotient_zero_gate, .quotient_no_commitments, .t_commitments
//   open, linearise                                 circ_p.evals, circ_p.w, circ_p.linearise.*
//   check_open_sizes                                circ_p.open_sizes, circ_p.open_sizes.wires / .z / .pi
//   column_device, open_device                      circ_p.column_len, .column_sigma0, .column_coset_len, circ_p.open_device.*
//   verify                                          <c>.verify, .verify_alpha_beta_swapped, .verify_wrong_value, .verify_sizes
//   prove, proof_challenges                         <c>.proof, <c>.challenges
//   verify_proof                                    <c>.verify_proof, .verify_proof_flipped, .verify_proof_short
//   Circuit(Circuit&&), operator=(Circuit&&)        <c>.move_ctor.*, <c>.move_assign.*
// Error, check                                     too_long.*, and every *.status / *.what record
#include <cstdio>
#include <fstream>
#include <functional>
#include <map>

#include "kzg_mi355x.hpp"

using namespace kzg_api;
using G2 = std::array<uint64_t, 36>;
using Bytes = std::vector<uint8_t>;

static std::map<std::string, Bytes> g_in;
static std::vector<std::pair<std::string, Bytes>> g_out;

static void read_records(const char* path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot read the input file");
    uint64_t len;
    while (f.read(reinterpret_cast<char*>(&len), 8)) {
        std::string name(len, '\0');
        f.read(&name[0], (std::streamsize)len);
        f.read(reinterpret_cast<char*>(&len), 8);
        Bytes data(len);
        f.read(reinterpret_cast<char*>(data.data()), (std::streamsize)len);
        if (!f) throw std::runtime_error("truncated input file");
        g_in[name] = std::move(data);
    }
}
static void write_records(const char* path) {
    std::ofstream f(path, std::ios::binary);
    for (const auto& r : g_out) {
        uint64_t len = r.first.size();
        f.write(reinterpret_cast<const char*>(&len), 8);
        f.write(r.first.data(), (std::streamsize)len);
        len = r.second.size();
        f.write(reinterpret_cast<const char*>(&len), 8);
        f.write(reinterpret_cast<const char*>(r.second.data()), (std::streamsize)len);
    }
    if (!f.flush()) throw std::runtime_error("cannot write the output file");
}
static const Bytes& in_bytes(const std::string& name) {
    const auto it = g_in.find(name);
    if (it == g_in.end()) throw std::runtime_error("no input record " + name);
    return it->second;
}
template <class T>
static std::vector<T> in_vec(const std::string& name) {
    const Bytes& b = in_bytes(name);
    if (b.size() % sizeof(T)) throw std::runtime_error("input record " + name + " has a ragged length");
    std::vector<T> v(b.size() / sizeof(T));
    if (!b.empty()) std::memcpy(static_cast<void*>(v.data()), b.data(), b.size());
    return v;
}
static std::vector<Scalar> in_scalars(const std::string& name) { return in_vec<Scalar>(name); }
static Scalar in_scalar(const std::string& name) { return in_vec<Scalar>(name).at(0); }

static void put(const std::string& name, const void* p, size_t bytes) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    g_out.emplace_back(name, bytes ? Bytes(b, b + bytes) : Bytes());
}
static void put(const std::string& name, const Scalar& s) { put(name, s.l.data(), 32); }
static void put(const std::string& name, const G1Point& p) { put(name, p.p1.data(), 144); }
static void put(const std::string& name, const std::vector<Scalar>& v) { put(name, v.data(), 32 * v.size()); }
static void put(const std::string& name, const std::vector<G1Point>& v) { put(name, v.data(), 144 * v.size()); }
static void put(const std::string& name, const Bytes& v) { put(name, v.data(), v.size()); }
static void put_u64(const std::string& name, uint64_t v) { put(name, &v, 8); }
static void put_bool(const std::string& name, bool v) { put_u64(name, v ? 1 : 0); }
// <name>.status: 0 when nothing was thrown, else Error::status; <name>.what: the text
static void put_throw(const std::string& name, const std::function<void()>& f) {
    int64_t status = 0;
    std::string what;
    try {
        f();
    } catch (const Error& e) {
        status = e.status;
        what = e.what();
    }
    put(name + ".status", &status, 8);
    put(name + ".what", what.data(), what.size());
}
static std::vector<Scalar> head(const std::vector<Scalar>& v, size_t n) { return std::vector<Scalar>(v.begin(), v.begin() + n); }
static std::vector<Scalar> slice(const std::vector<Scalar>& v, size_t at, size_t n) {
    return std::vector<Scalar>(v.begin() + at, v.begin() + at + n);
}
static Scalar bump(Scalar s) {  // another field element: the image with its low bit flipped stays below r for the test's values
    s.l[0] ^= 1;
    return s;
}

static void setup_cases(const SetupArtifacts& setup, const std::array<uint8_t, 32>& secret) {
    put_u64("srs.len", setup.len());
    put("srs.read_0_1", setup.read_g1(0, 1));
    put("srs.read_3_13", setup.read_g1(3, 13));
    put("srs.read_79_1", setup.read_g1(79, 1));
    for (uint64_t j = 0; j < 3; j++) put("g2." + std::to_string(j), SetupArtifacts::g2_at(secret, j).data(), 288);
    {
        SetupArtifacts small(0);
        small.generate(secret, 16);
        put_u64("srs16.len", small.len());
        put("srs16.first0", small.read_g1(0, 16));
        small.generate(secret, 16, 5);
        const std::vector<G1Point> from5 = small.read_g1(0, 16);
        put("srs16.first5", from5);
        // the other ways in, each read back: blst_p1 with a stride, 48-byte points, the binary cache
        struct Artifact { G1Point g1; G2 g2; };
        std::vector<Artifact> pairs(16);
        Bytes c48;
        for (size_t i = 0; i < 16; i++) {
            pairs[i].g1 = from5[i];
            const auto c = from5[i].compress();
            c48.insert(c48.end(), c.begin(), c.end());
        }
        SetupArtifacts io(0);
        io.load(&pairs[0].g1, sizeof(Artifact), 16);
        put("srs_io.load", io.read_g1(0, 16));
        io.generate(secret, 4);
        io.load_compressed(c48.data(), 16);
        put("srs_io.load_compressed", io.read_g1(0, 16));
        const std::string path = std::string(reinterpret_cast<const char*>(in_bytes("cache_path").data()), in_bytes("cache_path").size());
        io.save(path);
        io.generate(secret, 4);
        io.load_file(path);
        put("srs_io.load_file", io.read_g1(0, 16));
        put_u64("srs_io.len", io.len());
        SetupArtifacts multi(std::vector<int>{0, 0}, true);  // the multi-device constructor: two slices of one GPU, SRS replicated
        multi.generate(secret, 16, 5);
        put_u64("srs_io.multi.len", multi.len());
        put("srs_io.multi.commit", Polynomial::try_from(in_scalars("c16")).commit(multi));
    }
}

static void polynomial_cases(SetupArtifacts& setup, const G2& s_g2) {
    const std::vector<Scalar> c40 = in_scalars("c40"), pts = in_scalars("pts");
    const Polynomial p = Polynomial::try_from(c40);
    put_u64("try_from.full.len", p.coefficients().size());
    put_u64("try_from.full.degree", p.degree());
    const Polynomial padded = Polynomial::try_from(in_scalars("c40_top9_zero"));
    put("try_from.padded.coefficients", padded.coefficients());
    put_u64("try_from.padded.degree", padded.degree());
    put_u64("try_from.zeros.len", Polynomial::try_from(std::vector<Scalar>(3)).coefficients().size());
    put_u64("try_from.empty.len", Polynomial::try_from({}).coefficients().size());
    put_u64("try_from.empty.degree", Polynomial::try_from({}).degree());

    const G1Point cm = p.commit(setup);
    put("p40.commit", cm);
    const auto cm48 = cm.compress();
    put("p40.commit48", cm48.data(), 48);
    const Scalar z = pts[0], y = p.evaluate_at(z, setup);
    put("p40.eval", y);
    const Evaluation ev{z, y};
    const G1Point proof = ev.generate_proof(p, setup);
    put("p40.proof", proof);
    put("p40.add", cm.add(proof));
    put_bool("p40.verify", ev.verify_proof(proof, cm, s_g2.data()));
    put_bool("p40.verify_wrong_value", Evaluation{z, bump(y)}.verify_proof(proof, cm, s_g2.data()));
    put_bool("p40.verify_swapped", ev.verify_proof(cm, proof, s_g2.data()));
    put_bool("p40.commit_is_infinity", cm.is_infinity());
    put_bool("scalar.ops", Scalar{}.is_zero() && !z.is_zero() && z == pts[0] && !(z == pts[1]));

    // a constant polynomial: its proof is the point at infinity; a false claim is the library's status
    const Polynomial constant = Polynomial::try_from(head(c40, 1));
    const G1Point inf = Evaluation{z, c40[0]}.generate_proof(constant, setup);
    put("const.proof", inf);
    put_bool("const.proof_is_infinity", inf.is_infinity());
    put_bool("const.verify", Evaluation{z, c40[0]}.verify_proof(inf, constant.commit(setup), s_g2.data()));
    put_throw("const.false_claim", [&] { (void)Evaluation{z, bump(c40[0])}.generate_proof(constant, setup); });
    put_throw("false_claim", [&] { (void)Evaluation{z, bump(y)}.generate_proof(p, setup); });
    put_throw("too_long", [&] { (void)Polynomial::try_from(in_scalars("c81")).commit(setup); });

    // 3 polynomials of 40 coefficients, three per pass
    put_u64("srs.max_batch", setup.set_max_batch(3));
    const std::vector<Scalar> c3 = in_scalars("c3x40");
    put("batch.commit", commit_batch(setup, c3, 40));
    std::vector<Scalar> ys;
    for (size_t b = 0; b < 3; b++) ys.push_back(Polynomial::try_from(slice(c3, 40 * b, 40)).evaluate_at(pts[b], setup));
    std::vector<int> statuses;
    put("batch.open", open_batch(setup, c3, 40, head(pts, 3), ys, statuses));
    ys[1] = bump(ys[1]);
    const std::vector<G1Point> partly = open_batch(setup, c3, 40, head(pts, 3), ys, statuses);
    put("batch.open_one_wrong.0", partly[0]);
    put("batch.open_one_wrong.2", partly[2]);
    put("batch.open_one_wrong.statuses", statuses.data(), sizeof(int) * statuses.size());
    put_u64("srs.max_batch_back", setup.set_max_batch(1));
}

static void domain_cases(const SetupArtifacts& setup) {
    put("domain.root6", Domain::root(6));
    put("domain.root0", Domain::root(0));
    const std::vector<Scalar> v64 = in_scalars("v64");
    for (size_t n : {(size_t)1, (size_t)2, (size_t)64}) {
        put("domain.ntt." + std::to_string(n), Domain::ntt(head(v64, n), false, setup));
        put("domain.intt." + std::to_string(n), Domain::ntt(head(v64, n), true, setup));
    }
    put("domain.commit", Domain::commit(v64, setup));
    const Polynomial p = Polynomial::try_from(Domain::ntt(v64, true, setup));
    const Scalar z_out = in_scalar("z_out"), z_in = in_scalar("z_in3");  // z_in3 = w_64^3
    put("domain.proof_outside", Domain::generate_proof(v64, z_out, p.evaluate_at(z_out, setup), setup));
    put("domain.proof_inside", Domain::generate_proof(v64, z_in, v64[3], setup));
    put_throw("domain.false_claim", [&] { (void)Domain::generate_proof(v64, z_in, v64[4], setup); });
}

static void points_cases(const SetupArtifacts& setup, const std::vector<G2>& g2) {
    const Polynomial p = Polynomial::try_from(in_scalars("c40"));
    const G1Point cm = p.commit(setup);
    const std::vector<Scalar> pts = in_scalars("pts");
    for (size_t k : {(size_t)1, (size_t)4, (size_t)5}) {
        const std::string name = "pts" + std::to_string(k);
        Evaluations ev = Evaluations::at(p, head(pts, k), setup);
        put(name + ".results", ev.results);
        const G1Point proof = ev.generate_proof(p, setup);
        put(name + ".proof", proof);
        put(name + ".quotient", ev.quotient(p, setup));
        const std::vector<G1Point> g1 = setup.read_g1(0, k);
        const std::vector<G2> g2k(g2.begin(), g2.begin() + k + 1);
        put_bool(name + ".verify", ev.verify_proof(proof, cm, g1, g2k));
        ev.results[k - 1] = bump(ev.results[k - 1]);
        put_bool(name + ".verify_wrong_value", ev.verify_proof(proof, cm, g1, g2k));
        put_throw(name + ".false_claim", [&] { (void)ev.generate_proof(p, setup); });
    }
    // combined: 3 polynomials at one point
    const std::vector<Scalar> c3 = in_scalars("c3x40");
    const Scalar gamma = in_scalar("gamma");
    CombinedOpening co = open_combined(setup, c3, 40, pts[0], gamma);
    put("combined.results", co.results);
    put("combined.proof", co.proof);
    const std::vector<G1Point> cms = commit_batch(setup, c3, 40);
    put_bool("combined.verify", verify_combined(co, cms, g2[1].data()));
    co.results[2] = bump(co.results[2]);
    put_bool("combined.verify_wrong_value", verify_combined(co, cms, g2[1].data()));

    // point sets: examples/open_sets.cpp's shape; then a three-point set first and a single-point set last
    const auto run = [&](const std::string& name, const std::vector<Scalar>& coeffs, std::vector<uint32_t> set_of,
                         std::vector<std::vector<Scalar>> sets, size_t distinct, size_t longest) {
        SetsOpening so = open_sets(setup, coeffs, 40, std::move(set_of), std::move(sets), gamma);
        for (size_t i = 0; i < so.results.size(); i++) put(name + ".results." + std::to_string(i), so.results[i]);
        put(name + ".proof", so.proof);
        const std::vector<uint32_t> len = so.set_len();
        put(name + ".set_len", len.data(), 4 * len.size());
        put(name + ".flat_points", so.flat_points());
        const std::vector<G1Point> own = commit_batch(setup, coeffs, 40), g1 = setup.read_g1(0, longest);
        const std::vector<G2> g2t(g2.begin(), g2.begin() + distinct + 1);
        put_bool(name + ".verify", verify_sets(so, own, g1, g2t));
        so.results.back().back() = bump(so.results.back().back());
        put_bool(name + ".verify_wrong_value", verify_sets(so, own, g1, g2t));
    };
    run("sets_a", c3, {0, 1, 0}, {{pts[0]}, {pts[0], pts[1]}}, 2, 2);
    run("sets_b", head(c3, 80), {1, 0}, {{pts[0], pts[1], pts[2]}, {pts[3]}}, 4, 3);
}

static void cell_cases(const SetupArtifacts& setup, const std::vector<G2>& g2) {
    const Polynomial p = Polynomial::try_from(in_scalars("c40"));
    const std::vector<Scalar> v32 = head(in_scalars("v64"), 32);
    const unsigned shapes[][2] = {{6, 2}, {6, 0}, {6, 6}};
    for (const auto& s : shapes) {
        const std::string name = "cells." + std::to_string(s[0]) + "_" + std::to_string(s[1]);
        const Cells a = Cells::of(p, s[0], s[1], setup);
        put(name + ".values", a.values);
        put(name + ".proofs", a.proofs);
        const Cells b = Cells::of_evaluations(v32, s[0], s[1], setup);
        put(name + ".ev_values", b.values);
        put(name + ".ev_proofs", b.proofs);
    }
    // cells longer than the domain: the header sizes one proof, the library refuses the shape
    put_throw("cells.3_4", [&] { (void)Cells::of(Polynomial::try_from(head(in_scalars("c40"), 5)), 3, 4, setup); });
    put_throw("cells.3_4.ev", [&] { (void)Cells::of_evaluations(head(v32, 4), 3, 4, setup); });

    const auto put_rows = [](const std::string& name, const std::vector<std::vector<Scalar>>& rows) {
        put_u64(name + ".count", rows.size());
        for (size_t j = 0; j < rows.size(); j++) put(name + "." + std::to_string(j), rows[j]);
    };
    put_rows("cellq.full", Cells::quotients(p, 6, 2, 0, 16, setup));
    put_rows("cellq.part", Cells::quotients(p, 6, 2, 5, 3, setup));
    put_rows("cellq.padded", Cells::quotients(Polynomial::try_from(in_scalars("c40_top9_zero")), 6, 2, 0, 16, setup));

    // FK20 over ragged lengths: every result is of()'s for that polynomial
    const std::vector<Scalar> c3 = in_scalars("c3x40");
    const std::vector<Polynomial> many{Polynomial::try_from(slice(c3, 0, 33)), Polynomial::try_from(slice(c3, 40, 17)),
                                       Polynomial::try_from(slice(c3, 80, 5))};
    Cells::prepare_fk20(33, 2, setup);
    const std::vector<Cells> fk = Cells::of_many_fk20(many, 6, 2, setup);
    put_u64("fk20.count", fk.size());
    for (size_t b = 0; b < fk.size(); b++) {
        const Cells one = Cells::of(many[b], 6, 2, setup);
        put("fk20.values." + std::to_string(b), fk[b].values);
        put("fk20.proofs." + std::to_string(b), fk[b].proofs);
        put("fk20.of.values." + std::to_string(b), one.values);
        put("fk20.of.proofs." + std::to_string(b), one.proofs);
    }

    // batch verification: 5 records over 2 commitments (polynomials 0 and 1 of the FK20 batch), l = 4
    const std::vector<G1Point> cms{many[0].commit(setup), many[1].commit(setup)};
    const std::vector<uint32_t> idx{0, 1, 1, 0, 1}, ids{3, 0, 15, 7, 7};
    std::vector<Scalar> values;
    std::vector<G1Point> proofs;
    for (size_t t = 0; t < 5; t++) {
        const Cells& from = fk[idx[t]];
        values.insert(values.end(), from.values.begin() + 4 * ids[t], from.values.begin() + 4 * ids[t] + 4);
        proofs.push_back(from.proofs[ids[t]]);
    }
    const std::vector<G2> g2l(g2.begin(), g2.begin() + 5), g2_short(g2.begin(), g2.begin() + 4);
    put_bool("vcells.verify", Cells::verify_batch(cms, idx, ids, values, proofs, 6, 2, g2l, setup));
    std::vector<Scalar> wrong = values;
    wrong[4 * 3 + 2] = bump(wrong[4 * 3 + 2]);
    put_bool("vcells.verify_wrong_value", Cells::verify_batch(cms, idx, ids, wrong, proofs, 6, 2, g2l, setup));
    put_bool("vcells.verify_empty", Cells::verify_batch({}, {}, {}, {}, {}, 6, 2, g2l, setup));
    put_throw("vcells.short_g2", [&] { (void)Cells::verify_batch(cms, idx, ids, values, proofs, 6, 2, g2_short, setup); });
    const std::vector<uint32_t> ids_brp = in_vec<uint32_t>("vcells.ids_brp");
    const Bytes c48 = in_bytes("vcells.commitments48"), p48 = in_bytes("vcells.proofs48");
    put_bool("vcells.bytes.natural", Cells::verify_batch_bytes(c48, idx, ids, in_bytes("vcells.cells_be"), p48, 6, 2, KZG_ORDER_NATURAL, g2l, setup));
    put_bool("vcells.bytes.brp",
             Cells::verify_batch_bytes(c48, idx, ids_brp, in_bytes("vcells.cells_be_brp"), p48, 6, 2, KZG_ORDER_BIT_REVERSED, g2l, setup));
    put_bool("vcells.bytes.natural_wrong_value",
             Cells::verify_batch_bytes(c48, idx, ids, in_bytes("vcells.cells_be_wrong"), p48, 6, 2, KZG_ORDER_NATURAL, g2l, setup));
    put_bool("vcells.bytes.brp_wrong_value",
             Cells::verify_batch_bytes(c48, idx, ids_brp, in_bytes("vcells.cells_be_brp_wrong"), p48, 6, 2, KZG_ORDER_BIT_REVERSED, g2l, setup));
    put_bool("vcells.bytes.brp_as_natural",
             Cells::verify_batch_bytes(c48, idx, ids_brp, in_bytes("vcells.cells_be_brp"), p48, 6, 2, KZG_ORDER_NATURAL, g2l, setup));
    put_throw("vcells.bytes.short_g2",
              [&] { (void)Cells::verify_batch_bytes(c48, idx, ids, in_bytes("vcells.cells_be"), p48, 6, 2, KZG_ORDER_NATURAL, g2_short, setup); });
}

static void wire_cases(const SetupArtifacts& setup, const std::vector<G2>& g2) {
    const std::vector<G2> g2two(g2.begin(), g2.begin() + 2);
    const std::vector<uint32_t> idx = in_vec<uint32_t>("wire.open.idx");
    const Bytes c48 = in_bytes("wire.open.commitments48"), zs = in_bytes("wire.open.zs_be"), ys = in_bytes("wire.open.ys_be"),
                p48 = in_bytes("wire.open.proofs48");
    put_bool("wire.openings", Wire::verify_openings(c48, idx, zs, ys, p48, g2two, setup));
    put_bool("wire.openings_wrong_value", Wire::verify_openings(c48, idx, zs, in_bytes("wire.open.ys_be_wrong"), p48, g2two, setup));
    put_bool("wire.openings_swapped", Wire::verify_openings(c48, idx, ys, zs, p48, g2two, setup));

    const Bytes blobs = in_bytes("wire.blobs.blobs_be"), bc48 = in_bytes("wire.blobs.commitments48"), bz = in_bytes("wire.blobs.zs_be"),
                bp48 = in_bytes("wire.blobs.proofs48");
    Bytes out_ys{1, 2, 3};
    put_bool("wire.blobs", Wire::verify_blobs(blobs, 8, KZG_ORDER_NATURAL, bc48, bz, bp48, g2two, setup));
    put_bool("wire.blobs_with_ys", Wire::verify_blobs(blobs, 8, KZG_ORDER_NATURAL, bc48, bz, bp48, g2two, setup, &out_ys));
    put("wire.blobs.ys_be", out_ys);
    put_bool("wire.blobs_brp", Wire::verify_blobs(in_bytes("wire.blobs.blobs_be_brp"), 8, KZG_ORDER_BIT_REVERSED, bc48, bz, bp48, g2two, setup, &out_ys));
    put("wire.blobs_brp.ys_be", out_ys);
    put_bool("wire.blobs_wrong_proof", Wire::verify_blobs(blobs, 8, KZG_ORDER_NATURAL, bc48, bz, in_bytes("wire.blobs.proofs48_swapped"), g2two, setup));
    put_throw("wire.blobs_empty", [&] { put_bool("wire.blobs_empty.valid", Wire::verify_blobs({}, 8, KZG_ORDER_NATURAL, {}, {}, {}, g2two, setup, &out_ys)); });
    put_u64("wire.blobs_empty.ys_len", out_ys.size());

    const Bytes pts48 = in_bytes("wire.points48");
    put("wire.uncompress", Wire::g1_uncompress_batch(pts48, false, setup));
    put("wire.uncompress_subgroup", Wire::g1_uncompress_batch(pts48, true, setup));
    put_throw("wire.uncompress_off_subgroup", [&] { (void)Wire::g1_uncompress_batch(in_bytes("wire.points48_torsion"), true, setup); });
    put("wire.uncompress_torsion_unchecked", Wire::g1_uncompress_batch(in_bytes("wire.points48_torsion"), false, setup));
    put_throw("wire.uncompress_empty", [&] { put_u64("wire.uncompress_empty.len", Wire::g1_uncompress_batch({}, true, setup).size()); });
    put("wire.fr", Wire::fr_from_bytes_batch(in_bytes("wire.fr_be"), setup));
    put_throw("wire.fr_not_below_r", [&] { (void)Wire::fr_from_bytes_batch(in_bytes("wire.fr_be_bad"), setup); });
    put_throw("wire.fr_empty", [&] { put_u64("wire.fr_empty.len", Wire::fr_from_bytes_batch({}, setup).size()); });
    put_throw("wire.fr_ragged", [&] { (void)Wire::fr_from_bytes_batch(Bytes(33), setup); });
}

// kzg_dev_alloc / kzg_dev_upload buffers for open_device, freed on the way out
struct DeviceBuffer {
    kzg_ctx* ctx;
    void* d = nullptr;
    DeviceBuffer(kzg_ctx* c, const std::vector<Scalar>& host) : ctx(c) {
        check(kzg_dev_alloc(ctx, 32 * host.size(), &d), ctx);
        check(kzg_dev_upload(ctx, d, host.data(), 32 * host.size()), ctx);
    }
    ~DeviceBuffer() { kzg_dev_free(ctx, d); }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
};

static void circuit_cases(const SetupArtifacts& setup, const std::string& name, size_t n, size_t t, unsigned log_ext, bool blinded,
                          const std::vector<G2>& g2) {
    const auto in = [&](const char* field) { return in_scalars(name + "." + field); };
    const std::vector<Scalar> q_lin = in("q_lin"), q_mul = in("q_mul"), q_const = in("q_const"), sigmas = in("sigmas"), shifts = in("shifts"),
                              wires = in("wires"), z = in("z"), pi = in("pi"), pub = in("public"), bl = in("blinders");
    const Scalar alpha = in("alpha")[0], beta = in("beta")[0], gamma = in("gamma")[0], zeta = in("zeta")[0], v = in("v")[0];
    const size_t e = (size_t)1 << log_ext;
    const G1Point g1 = setup.read_g1(0, 1)[0];
    const uint64_t* g2p = g2[0].data();  // 36 u64 each, back to back

    {
        Circuit bare(setup, q_lin, q_mul, q_const, sigmas, shifts, log_ext, false);
        put_u64(name + ".bare.key_len", bare.key().size());
        put_throw(name + ".bare.prove", [&] { (void)bare.prove(wires, pub, {}); });
        put(name + ".bare.quotient", bare.quotient(wires, z, alpha, beta, gamma, pi, {}, false).coeffs);
    }
    Circuit c(setup, q_lin, q_mul, q_const, sigmas, shifts, log_ext);
    put(name + ".key", c.key());
    put_u64(name + ".n", c.n());
    put_u64(name + ".t", c.t());
    put_u64(name + ".proof_size", Circuit::proof_size(t, log_ext));
    put_u64(name + ".blinders_len", c.blinders().size());

    // the rounds by hand under the oracle's challenges
    Circuit::Quotient q;
    Circuit::Opening o;
    std::vector<G1Point> wire_cm, z_cm;
    if (blinded) {
        wire_cm = c.commit_blinded(wires, t, bl.data(), 2);
        z_cm = c.commit_blinded(z, 1, bl.data() + 2 * t, 3);
        q = c.quotient_blinded(wires, z, alpha, beta, gamma, bl, pi);
        put(name + ".quotient_no_commitments", c.quotient_blinded(wires, z, alpha, beta, gamma, bl, pi, false).coeffs);
        o = c.open_blinded(wires, z, q.coeffs, alpha, beta, gamma, zeta, v, bl, pi);
        put_throw(name + ".open_sizes", [&] { (void)c.open_blinded(wires, z, head(q.coeffs, q.coeffs.size() - 1), alpha, beta, gamma, zeta, v, bl, pi); });
    } else {
        for (size_t j = 0; j < t; j++) wire_cm.push_back(Domain::commit(slice(wires, j * n, n), setup));
        z_cm.push_back(Domain::commit(z, setup));
        q = c.quotient(wires, z, alpha, beta, gamma, pi);
        put(name + ".quotient_no_commitments", c.quotient(wires, z, alpha, beta, gamma, pi, {}, false).coeffs);
        // the caller's own term on the coset, here zero: the same T
        put(name + ".quotient_zero_gate", c.quotient(wires, z, alpha, beta, gamma, pi, std::vector<Scalar>(e * n)).coeffs);
        o = c.open(wires, z, q.coeffs, alpha, beta, gamma, zeta, v, pi);
        const auto lin = c.linearise(wires, z, q.coeffs, alpha, beta, gamma, zeta, pi);
        put(name + ".linearise.evals", lin.first);
        put(name + ".linearise.r", lin.second);
        // check_open_sizes: the header's own Error, before any library call
        put_throw(name + ".open_sizes", [&] { (void)c.open(wires, z, head(q.coeffs, q.coeffs.size() - 1), alpha, beta, gamma, zeta, v, pi); });
        put_throw(name + ".open_sizes.wires", [&] { (void)c.open(head(wires, n * t - 1), z, q.coeffs, alpha, beta, gamma, zeta, v, pi); });
        put_throw(name + ".open_sizes.z", [&] { (void)c.linearise(wires, head(z, n - 1), q.coeffs, alpha, beta, gamma, zeta, pi); });
        put_throw(name + ".open_sizes.pi", [&] { (void)c.open(wires, z, q.coeffs, alpha, beta, gamma, zeta, v, head(pi, n - 1)); });
        // the device form: a resident column of the circuit's own as the first wire column's stand-in would change the proof,
        // so the resident sigma_0 values are read back through it instead, and the inputs go up with kzg_dev_upload
        const auto col = c.column_device(KZG_CIRCUIT_COL_SIGMA, KZG_CIRCUIT_VALUES);
        put_u64(name + ".column_len", col.second);
        std::vector<Scalar> resident(col.second);
        check(kzg_dev_download(setup.ctx(), resident.data(), col.first, 32 * resident.size()), setup.ctx());
        put(name + ".column_sigma0", resident);
        put_u64(name + ".column_coset_len", c.column_device(KZG_CIRCUIT_COL_L0, KZG_CIRCUIT_COSET).second);
        DeviceBuffer d_wires(setup.ctx(), wires), d_z(setup.ctx(), z), d_pi(setup.ctx(), pi), d_t(setup.ctx(), q.coeffs);
        const Circuit::Opening od = c.open_device(d_wires.d, n, d_z.d, d_pi.d, d_t.d, alpha, beta, gamma, zeta, v);
        put(name + ".open_device.evals", od.evals);
        put(name + ".open_device.proof", od.proof);
        // ... and with a resident column as an input: sigma_0's values where z is expected can only fail the linearisation
        put_throw(name + ".open_device.resident_as_z",
                  [&] { (void)c.open_device(d_wires.d, n, col.first, d_pi.d, d_t.d, alpha, beta, gamma, zeta, v); });
    }
    put(name + ".wire_commitments", wire_cm);
    put(name + ".z_commitment", z_cm);
    put(name + ".quotient", q.coeffs);
    put(name + ".t_commitments", q.commitments);
    put(name + ".evals", o.evals);
    put(name + ".w", o.proof);
    const auto verify = [&](const std::vector<Scalar>& evals, const Scalar& a, const Scalar& b) {
        return Circuit::verify(c.key(), n, log_ext, shifts, wire_cm, z_cm[0], q.commitments, pub, evals, a, b, gamma, zeta, v, o.proof, g1, g2p);
    };
    put_bool(name + ".verify", verify(o.evals, alpha, beta));
    put_bool(name + ".verify_alpha_beta_swapped", verify(o.evals, beta, alpha));
    std::vector<Scalar> wrong = o.evals;
    wrong[1] = bump(wrong[1]);
    put_bool(name + ".verify_wrong_value", verify(wrong, alpha, beta));
    put_throw(name + ".verify_sizes", [&] {
        (void)Circuit::verify(c.key(), n, log_ext, shifts, wire_cm, z_cm[0], std::vector<G1Point>(e), pub, o.evals, alpha, beta, gamma, zeta, v,
                              o.proof, g1, g2p);
    });

    // the proof in one call, its challenges and its verifier
    Bytes proof = c.prove(wires, pub, blinded ? bl : std::vector<Scalar>{});
    put(name + ".proof", proof);
    const auto ch = Circuit::proof_challenges(c.key(), n, log_ext, shifts, pub, proof);
    put(name + ".challenges", ch.data(), 32 * ch.size());
    put_bool(name + ".verify_proof", Circuit::verify_proof(c.key(), n, log_ext, shifts, pub, proof, g1, g2p));
    Bytes flipped = proof;
    flipped[48 * (t + e) + 5] ^= 1;  // inside the first evaluation
    put_bool(name + ".verify_proof_flipped", Circuit::verify_proof(c.key(), n, log_ext, shifts, pub, flipped, g1, g2p));
    flipped.pop_back();
    put_throw(name + ".verify_proof_short", [&] { (void)Circuit::verify_proof(c.key(), n, log_ext, shifts, pub, flipped, g1, g2p); });

    // moves: the moved-to object proves the same bytes, the moved-from handle is null, both are destroyed here
    const kzg_circuit* h = c.handle();
    Circuit moved(std::move(c));
    put_bool(name + ".move_ctor.handle", moved.handle() == h && c.handle() == nullptr && moved.n() == n && moved.t() == t);
    put(name + ".move_ctor.proof", moved.prove(wires, pub, blinded ? bl : std::vector<Scalar>{}));
    Circuit other(setup, q_lin, q_mul, q_const, sigmas, shifts, log_ext, false);
    other = std::move(moved);
    put_bool(name + ".move_assign.handle", other.handle() == h && moved.handle() == nullptr && other.key().size() == 2 * t + 2);
    put(name + ".move_assign.proof", other.prove(wires, pub, blinded ? bl : std::vector<Scalar>{}));
}

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <input records> <output records>\n", argv[0]);
        return 2;
    }
    try {
        read_records(argv[1]);
        const Bytes& sb = in_bytes("secret");
        std::array<uint8_t, 32> secret{};
        std::copy(sb.begin(), sb.begin() + 32, secret.begin());
        std::vector<G2> g2;
        for (uint64_t j = 0; j < 6; j++) g2.push_back(SetupArtifacts::g2_at(secret, j));
        {
            SetupArtifacts setup(0);
            setup.generate(secret, 80);
            setup_cases(setup, secret);
            polynomial_cases(setup, g2[1]);
            domain_cases(setup);
            points_cases(setup, g2);
            cell_cases(setup, g2);
            wire_cases(setup, g2);
            circuit_cases(setup, "circ_b", 8, 3, 2, true, g2);
            circuit_cases(setup, "circ_p", 16, 2, 2, false, g2);
        }
        put_u64("done", 1);  // every circuit and the context were destroyed before this record
        write_records(argv[2]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "hpp_parity: %s\n", e.what());
        return 1;
    }
    return 0;
}
