// Stand-alone host program (TEST INFRASTRUCTURE): the per-call functions of csrc/ecc_calls.hpp (and ecc_pair_stage1 of
// csrc/ecc_circuit.hpp, which they run behind) over exactly-sized heap buffers, built with -fsanitize=address,undefined by
// tests/test_ecc_calls_cpu.py and run as a child process.  Batches: a kind alone and all three, pairing ops of 0, 1 and 2 pairs with an
// empty op first, last and in the middle, words at the edges of p and 2^256.  A handful of results are compared with known values
// (2G, [r]G, e(G, Q) e(-G, Q) = 1); exit status 0 = no mismatch (the sanitizers abort on their own findings).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/zkevm_hip.h"
#include "../../zkevm_specs_amd/csrc/ecc_calls.hpp"

static const u64 W_P[4] = {0x3c208c16d87cfd47ull, 0x97816a916871ca8dull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
static const u64 W_R[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
static const u64 W_NEG2[4] = {0x3c208c16d87cfd45ull, 0x97816a916871ca8dull, 0xb85045b68181585dull, 0x30644e72e131a029ull};  // p - 2
static const u64 W_2G[2][4] = {{0xd3c208c16d87cfd3ull, 0xd97816a916871ca8ull, 0x9b85045b68181585ull, 0x030644e72e131a02ull},
                               {0xff3ebf7a5a18a2c4ull, 0x68a6a449e3538fc7ull, 0xe7845f96b2ae9c0aull, 0x15ed738c0e0a7c92ull}};
static const u64 W_Q[4][4] = {{0x97e485b7aef312c2ull, 0xf1aa493335a9e712ull, 0x7260bfb731fb5d25ull, 0x198e9393920d483aull},   // G2's x.c1
                              {0x46debd5cd992f6edull, 0x674322d4f75edaddull, 0x426a00665e5c4479ull, 0x1800deef121f1e76ull},   // x.c0
                              {0x55acdadcd122975bull, 0xbc4b313370b38ef3ull, 0xec9e99ad690c3395ull, 0x090689d0585ff075ull},   // y.c1
                              {0x4ce6cc0166fa7daaull, 0xe3d1e7690c43d37bull, 0x4aab71808dcb408full, 0x12c85ea5db8c6debull}};  // y.c0
static const u64 W_1[4] = {1, 0, 0, 0}, W_2[4] = {2, 0, 0, 0}, W_3[4] = {3, 0, 0, 0}, W_0[4] = {0, 0, 0, 0};
static const u64 W_MAX[4] = {~0ull, ~0ull, ~0ull, ~0ull};

static void put(std::vector<u64>& v, const u64* w) { v.insert(v.end(), w, w + 4); }
static void put_pair(std::vector<u64>& v, const u64* px, const u64* py, bool q_inf = false) {
    put(v, px);
    put(v, py);
    for (int k = 0; k < 4; k++) put(v, q_inf ? W_0 : W_Q[k]);
}
static bool is_word(const u64* c, const u64* w) { return memcmp(c, w, 32) == 0; }

// one pass over exactly-sized buffers; returns the number of calls whose outputs are not what `want_valid` / `want_out` say
static int run(const std::vector<u64>& add_in, const std::vector<u64>& mul_in, const std::vector<u64>& pair_pts, const std::vector<u32>& off,
               const std::vector<int>& want_valid, const std::vector<const u64*>& want_x, const char* what) {
    const u64 n_add = add_in.size() / 16, n_mul = mul_in.size() / 12, n_pr = off.size() - 1, np = n_add + n_mul, n = np + n_pr;
    const u64 rand[4] = {0x1234567, 0, 0, 0};
    zk_ecc_calls in = {n_add ? add_in.data() : nullptr, n_add, n_mul ? mul_in.data() : nullptr, n_mul, pair_pts.empty() ? nullptr : pair_pts.data(),
                       n_pr ? off.data() : nullptr, n_pr, rand};
    EccCallArgs a;
    memset(&a, 0, sizeof a);
    const char* err = nullptr;
    if (ecc_calls_check(&in, a, &err)) { fprintf(stderr, "ecc_calls_asan: %s: %s\n", what, err); return 1; }
    const u64 n_pp = n_pr ? off[n_pr] : 0;
    std::vector<u64> points(np * 24), pair_out(n_pr * 4), rows(n * ECL_ROW_WORDS), tcand(n * ECL_ROW_WORDS), aux(n * ECL_AUX_CELLS * 4);
    std::vector<u32> kind(n), flags(n_pp);
    std::vector<bn::Fq12> f(n_pp);
    a.add_in = in.add_in; a.mul_in = in.mul_in; a.pair_pts = in.pair_pts; a.pair_off = off.data();
    a.points = points.data(); a.pair_out = pair_out.data(); a.rows = rows.data(); a.tcand = tcand.data(); a.aux = aux.data();
    a.aux_kind = kind.data(); a.pair_flags = flags.data(); a.pair_f = f.data();
    for (u64 i = 0; i < np; i++) ecc_call_point(a, i);
    EccPairArgs pr{};
    pr.a.pair_pts = a.pair_pts;
    pr.pair_flags = a.pair_flags;
    pr.pair_f = a.pair_f;
    for (u64 t = 0; t < n_pp; t++) ecc_pair_stage1(pr, (u32)t);
    for (u64 k = 0; k < n_pr; k++) ecc_call_pairing(a, k);
    int bad = 0;
    for (u64 i = 0; i < n; i++) {
        const u64* row = &rows[i * ECL_ROW_WORDS];
        const u64 want_kind = i < n_add ? 6 : i < np ? 7 : 8;
        bool ok = row[0] == want_kind - 5 && kind[i] == want_kind && row[48] == (u64)want_valid[i] && (row[49] | row[50] | row[51]) == 0;
        ok = ok && is_word(row + 4 * (i < np ? 10 : 11), want_x[i]);
        ok = ok && ecl_row_eq(row, &tcand[i * ECL_ROW_WORDS]);  // (every result here is below the scalar modulus)
        if (i < np) ok = ok && is_word(&points[i * 24 + 16], want_x[i]) && is_word(&aux[i * ECL_AUX_CELLS * 4 + 4 * (i < n_add ? 8 : 6)], want_x[i]);
        else ok = ok && is_word(&pair_out[(i - np) * 4], want_x[i]) && aux[i * ECL_AUX_CELLS * 4 + 4] == off[i - np + 1] - off[i - np] && is_word(&aux[i * ECL_AUX_CELLS * 4 + 12], want_x[i]);
        if (!ok) { fprintf(stderr, "ecc_calls_asan: %s: call %llu\n", what, (unsigned long long)i); bad++; }
    }
    return bad;
}

static int run_rejections() {
    int bad = 0;
    EccCallArgs a;
    const char* err;
    const u64 rand[4] = {1, 0, 0, 0};
    u32 off_bad0[2] = {1, 1}, off_dec[3] = {0, 1, 0}, off_big[2] = {0, 1u << 31}, off_ok[2] = {0, 0};
    zk_ecc_calls in = {nullptr, 0, nullptr, 0, W_P, off_bad0, 1, rand};
    bad += ecc_calls_check(&in, a, &err) != ZK_ERR_ECL_OFFSETS;
    in.pair_off = off_dec; in.n_pairing = 2;
    bad += ecc_calls_check(&in, a, &err) != ZK_ERR_ECL_OFFSETS;
    in.pair_off = off_big; in.n_pairing = 1;
    bad += ecc_calls_check(&in, a, &err) != ZK_ERR_ECL_ROWS;
    in.pair_off = off_ok;
    bad += ecc_calls_check(&in, a, &err) != 0;
    in.randomness = W_R;
    bad += ecc_calls_check(&in, a, &err) != ZK_ERR_ECL_RANDOMNESS;
    in.randomness = rand; in.n_add = 1ull << 31;
    bad += ecc_calls_check(&in, a, &err) != ZK_ERR_ECL_ROWS;
    in.n_add = 0; in.n_pairing = 0;
    bad += ecc_calls_check(&in, a, &err) != -1;
    if (bad) fprintf(stderr, "ecc_calls_asan: %d rejection mismatches\n", bad);
    return bad;
}

int main() {
    std::vector<u64> adds, muls, pts;
    // adds: G + G = 2G; O + O = O; G + (1, 3) invalid; (2^256 - 1, 2) + G invalid; G + (-G) = O
    const u64* add_words[5][4] = {{W_1, W_2, W_1, W_2}, {W_0, W_0, W_0, W_0}, {W_1, W_2, W_1, W_3}, {W_MAX, W_2, W_1, W_2}, {W_1, W_2, W_1, W_NEG2}};
    for (auto& c : add_words)
        for (const u64* w : c) put(adds, w);
    // muls: [2]G = 2G; [r]G = O; [r + ... 2^256 - 1]G valid (the full-width chain); [2](p, 2) invalid; [0]G = O
    const u64* mul_words[5][3] = {{W_1, W_2, W_2}, {W_1, W_2, W_R}, {W_1, W_2, W_MAX}, {W_P, W_2, W_2}, {W_1, W_2, W_0}};
    for (auto& c : mul_words)
        for (const u64* w : c) put(muls, w);
    // pairings: (), (G, Q)(-G, Q) = 1, (G, Q) = 0, (), ((1, 3), Q) invalid, (G, inf) = 1, ()
    put_pair(pts, W_1, W_2);
    put_pair(pts, W_1, W_NEG2);
    put_pair(pts, W_1, W_2);
    put_pair(pts, W_1, W_3);
    put_pair(pts, W_1, W_2, true);
    const std::vector<u32> off = {0, 0, 2, 3, 3, 4, 5, 5};
    const std::vector<int> v_add = {1, 1, 0, 0, 1}, v_mul = {1, 1, 1, 0, 1}, v_pr = {1, 1, 1, 1, 0, 1, 1};
    const std::vector<const u64*> x_add = {W_2G[0], W_0, W_0, W_0, W_0}, x_pr = {W_1, W_1, W_0, W_1, W_0, W_1, W_1};
    int bad = 0;
    bad += run(adds, {}, {}, {0}, v_add, x_add, "adds");
    bad += run({}, {}, pts, off, v_pr, x_pr, "pairings");
    {   // the muls alone first, to learn [2^256 - 1]G's x from the run itself: it must be on no list of special values
        std::vector<u64> one(muls.begin() + 24, muls.begin() + 36);
        EccCallArgs a;
        memset(&a, 0, sizeof a);
        std::vector<u64> points(24), rows(ECL_ROW_WORDS), tcand(ECL_ROW_WORDS), aux(ECL_AUX_CELLS * 4);
        std::vector<u32> kind(1);
        a.mul_in = one.data(); a.n_mul = 1; a.points = points.data(); a.rows = rows.data(); a.tcand = tcand.data(); a.aux = aux.data(); a.aux_kind = kind.data();
        ecc_call_point(a, 0);
        static u64 x_max[4];
        memcpy(x_max, &points[16], 32);
        bad += is_word(x_max, W_0) || is_word(x_max, W_1) || is_word(x_max, W_2G[0]);
        const std::vector<const u64*> x_mul = {W_2G[0], W_0, x_max, W_0, W_0};
        bad += run({}, muls, {}, {0}, v_mul, x_mul, "muls");
        std::vector<int> v_all(v_add);
        v_all.insert(v_all.end(), v_mul.begin(), v_mul.end());
        v_all.insert(v_all.end(), v_pr.begin(), v_pr.end());
        std::vector<const u64*> x_all(x_add);
        x_all.insert(x_all.end(), x_mul.begin(), x_mul.end());
        x_all.insert(x_all.end(), x_pr.begin(), x_pr.end());
        bad += run(adds, muls, pts, off, v_all, x_all, "all");
    }
    bad += run_rejections();
    printf("ecc_calls_asan: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
