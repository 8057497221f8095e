// Stand-alone host program (TEST INFRASTRUCTURE): the per-element functions of csrc/block_tables.hpp over exactly-sized heap buffers,
// built with -fsanitize=address,undefined by tests/test_block_tables_cpu.py and run as a child process.  Shapes: calldata lengths at
// the edges of the 16-byte pieces and of the gas kernel's block, the calldata 0, 1, 3, 7, 8 and 9 bytes past an aligned address (the
// bytes in front of it poisoned where a whole granule is), empty txs, no txs, history of 0 / 1 / 256 hashes, a block number that crosses
// p.  Every row is compared with a row-by-row construction; exit status 0 = no mismatch (the sanitizers abort on their own findings).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <sanitizer/asan_interface.h>
#include "../../zkevm_specs_amd/csrc/block_tables.hpp"

static u64 rnd_state = 0x9e3779b97f4a7c15ull;
static u64 rnd() {
    rnd_state ^= rnd_state << 13; rnd_state ^= rnd_state >> 7; rnd_state ^= rnd_state << 17;
    return rnd_state;
}
// v mod p by repeated subtraction on 64-bit limbs (independent of btb_reduce's 32-bit form)
static void mod_p(const u64* v, u64* out) {
    memcpy(out, v, 32);
    while (!btbh_lt(out, BTB_P64)) btbh_sub(out, out, BTB_P64);
}
static bool cell_is(const u64* c, u64 a, u64 b, u64 d, u64 e) { return c[0] == a && c[1] == b && c[2] == d && c[3] == e; }

static int run(const std::vector<u32>& lengths, u32 mis, u64 n_hist, u64 n_wd, bool has_block, const u64* number_in = nullptr, int fill = -1) {
    const u64 n = lengths.size();
    std::vector<u64> offs(n + 1, 0);
    for (u64 i = 0; i < n; i++) offs[i + 1] = offs[i] + lengths[i];
    const u64 n_bytes = offs[n];
    uint8_t* buf = (uint8_t*)aligned_alloc(16, ((mis + n_bytes + 15) / 16 + 1) * 16);  // (freed below; the tail past mis + n_bytes is poisoned)
    uint8_t* cd = buf + mis;
    for (u64 k = 0; k < n_bytes; k++) cd[k] = fill >= 0 ? (uint8_t)fill : (uint8_t)((rnd() % 3) ? rnd() : 0);
    const size_t whole = ((mis + n_bytes + 15) / 16 + 1) * 16;
    ASAN_POISON_MEMORY_REGION(buf + mis + n_bytes, whole - mis - n_bytes);
    if (mis >= 8) ASAN_POISON_MEMORY_REGION(buf, 8);
    std::vector<u64> txf(n * 36), ids(n * 4), block(has_block ? 32 : 0), hashes(n_hist * 4), wd(n_wd * 16), wd_ids(n_wd * 4);
    std::vector<u32> to_none(n), access(2 * n);
    for (u64 i = 0; i < n; i++) {
        for (int k = 0; k < 36; k++) txf[i * 36 + k] = rnd();
        txf[i * 36 + 0] = 3 * i + 1; txf[i * 36 + 1] = txf[i * 36 + 2] = txf[i * 36 + 3] = 0;  // ascending canonical ids
        if (i % 3 == 0) for (int k = 0; k < 4; k++) txf[i * 36 + 4 * BTB_F_NONCE + k] = ~0ull;  // 2^256 - 1: five subtractions
        memcpy(&ids[4 * i], &txf[i * 36], 32);
        to_none[i] = (u32)(rnd() & 1);
        access[2 * i] = (u32)(rnd() % 5); access[2 * i + 1] = (u32)(rnd() % 9);
    }
    for (auto& x : block) x = rnd();
    for (auto& x : hashes) x = rnd();
    if (has_block) {
        u64 num[4] = {n_hist + 41, 0, 0, 0};
        memcpy(&block[8], number_in ? number_in : num, 32);
    }
    for (u64 i = 0; i < n_wd; i++) {
        for (int k = 0; k < 16; k++) wd[i * 16 + k] = rnd();
        wd[i * 16] = 7 * i; wd[i * 16 + 1] = wd[i * 16 + 2] = wd[i * 16 + 3] = 0;
        memcpy(&wd_ids[4 * i], &wd[i * 16], 32);
    }
    BtbPlan z;
    char msg[256];
    const int rc = btb_plan(txf.data(), offs.data(), n, has_block ? block.data() : nullptr, n_hist, wd.data(), n_wd, mis, z, msg, sizeof msg);
    if (rc) { fprintf(stderr, "block_tables_asan: plan failed: %s\n", msg); return 1; }
    std::vector<u32> part(z.n_gas_blocks), pre(z.n_gas_blocks + 1), tx_flags(z.n_tx_rows), blk_flags(z.n_block_rows);
    std::vector<u64> tx(z.n_tx_rows * 20), blk(z.n_block_rows * 16), wdt(n_wd * 16);
    BtbArgs a;
    memset(&a, 0, sizeof a);
    a.txf = txf.data(); a.to_none = to_none.data(); a.access = access.data(); a.calldata = cd; a.offs = offs.data(); a.ids = ids.data();
    a.block = block.data(); a.hashes = hashes.data(); a.wd = wd.data(); a.wd_ids = wd_ids.data();
    a.n_txs = n; a.n_bytes = n_bytes; a.n_tx_rows = z.n_tx_rows; a.n_hist = n_hist; a.n_block_rows = z.n_block_rows; a.n_wd = n_wd;
    if (has_block) memcpy(a.number, &block[8], 32);
    a.mis = mis; a.hist_rot = z.hist_rot; a.n_gas_blocks = z.n_gas_blocks;
    a.gas_part = part.data(); a.gas_pre = pre.data(); a.tx = tx.data(); a.tx_flags = tx_flags.data(); a.blk = blk.data(); a.blk_flags = blk_flags.data();
    a.wdt = wdt.data();
    for (u64 b = 0; b < a.n_gas_blocks; b++) a.gas_part[b] = btb_gas_block(a, b);
    btb_gas_prefix(a);
    for (u64 row = 0; row < a.n_tx_rows; row++) {
        const u64 i = btb_tx_of_row(a, row, 0);
        for (u32 q = 0; q < BTB_TX_PIECES; q++) btb_tx_piece(a, i, offs[i], offs[i + 1], row, q, a.tx[(row * 10 + q) * 2], a.tx[(row * 10 + q) * 2 + 1]);
        a.tx_flags[row] = btb_tx_flag(i, offs[i], row);
    }
    // the per-wavefront index of the device's row writer against the search it stands for
    std::vector<u32> wave_tx((z.n_tx_rows * 10 + 63) / 64);
    btb_wave_index(offs.data(), n, z.n_tx_rows, wave_tx.data());
    int bad_index = 0;
    for (u64 w = 0; w < wave_tx.size(); w++) bad_index += wave_tx[w] != btb_tx_of_row(a, 64 * w / 10, 0);
    for (u64 r = 0; r < a.n_block_rows; r++) btb_block_row(a, r);
    for (u64 r = 0; r < a.n_wd; r++) btb_wd_row(a, r);
    // the row-by-row construction
    int bad = bad_index;
    u64 row = 0;
    for (u64 i = 0; i < n; i++) {
        const u64* f = &txf[i * 36];
        u64 gas = 0;
        for (u64 k = offs[i]; k < offs[i + 1]; k++) gas += cd[k] ? 16 : 4;
        for (u64 t = 0; t < 12 + (u64)lengths[i]; t++, row++) {
            const u64* r = &tx[row * 20];
            bad += !cell_is(r, f[0], 0, 0, 0) || !cell_is(r + 4, t < 12 ? t + 1 : 13, 0, 0, 0) || !cell_is(r + 8, t < 12 ? 0 : t - 12, 0, 0, 0);
            u64 lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
            u32 flag = 0;
            const int word_field[12] = {-1, -1, BTB_F_GAS_PRICE, BTB_F_CALLER, BTB_F_CALLEE, -1, BTB_F_VALUE, -1, -1, -1, -1, -1};
            const int fq_field[12] = {BTB_F_NONCE, BTB_F_GAS, -1, -1, -1, -1, -1, -1, -1, BTB_F_INVALID, -1, BTB_F_SIGN_HASH};
            if (t >= 12) lo[0] = cd[offs[i] + t - 12];
            else if (word_field[t] >= 0) { lo[0] = f[4 * word_field[t]]; lo[1] = f[4 * word_field[t] + 1]; hi[0] = f[4 * word_field[t] + 2]; hi[1] = f[4 * word_field[t] + 3]; flag = 1; }
            else if (fq_field[t] >= 0) mod_p(f + 4 * fq_field[t], lo);
            else if (t == 5) lo[0] = to_none[i] ? 1 : 0;
            else if (t == 7) lo[0] = lengths[i];
            else if (t == 8) lo[0] = gas;
            else lo[0] = 2400ull * access[2 * i] + 1900ull * access[2 * i + 1];
            bad += memcmp(r + 12, lo, 32) != 0 || memcmp(r + 16, hi, 32) != 0 || tx_flags[row] != flag;
        }
    }
    bad += row != z.n_tx_rows;
    if (has_block) {
        bad += z.n_block_rows != 8 + n_hist;
        u64 prev[4] = {0, 0, 0, 0};
        for (u64 r = 0; r < z.n_block_rows; r++) {
            const u64* o = &blk[r * 16];
            const bool hist = r >= 7 && r < 7 + n_hist;
            bad += o[0] != (r < 7 ? r + 1 : (hist ? 8 : 9)) || o[1] || o[2] || o[3];
            if (hist) {
                if (r > 7) bad += !btbh_lt(prev, o + 4);  // ascending number cells
                memcpy(prev, o + 4, 32);
                // the hash this row carries is the one whose number cell it shows: number - n_hist + j == cell (mod p)
                bool found = false;
                for (u64 j = 0; j < n_hist && !found; j++) {
                    u64 d[4], m[4];
                    const u64 back[4] = {n_hist - j, 0, 0, 0};
                    btbh_sub(d, a.number, back);
                    mod_p(d, m);
                    found = memcmp(m, o + 4, 32) == 0 && o[8] == hashes[4 * j] && o[9] == hashes[4 * j + 1] && o[12] == hashes[4 * j + 2] && o[13] == hashes[4 * j + 3];
                }
                bad += !found || blk_flags[r] != 1;
            } else {
                const u64 src = r < 7 ? r : 7;
                const bool word = r == 0 || r == 4 || r == 5;
                u64 m[4];
                mod_p(&block[4 * src], m);
                bad += !cell_is(o + 4, 0, 0, 0, 0) || blk_flags[r] != (word ? 1u : 0u);
                if (word) bad += !cell_is(o + 8, block[4 * src], block[4 * src + 1], 0, 0) || !cell_is(o + 12, block[4 * src + 2], block[4 * src + 3], 0, 0);
                else bad += memcmp(o + 8, m, 32) != 0 || !cell_is(o + 12, 0, 0, 0, 0);
            }
        }
    }
    for (u64 r = 0; r < n_wd; r++)
        for (int c = 0; c < 4; c++) {
            u64 m[4];
            mod_p(&wd[r * 16 + 4 * c], m);
            bad += memcmp(&wdt[r * 16 + 4 * c], m, 32) != 0;
        }
    ASAN_UNPOISON_MEMORY_REGION(buf, whole);
    free(buf);
    if (bad) fprintf(stderr, "block_tables_asan: %d mismatches (%llu txs, %llu bytes, mis %u, %llu hashes)\n", bad, (unsigned long long)n,
                     (unsigned long long)n_bytes, mis, (unsigned long long)n_hist);
    return bad;
}

int main() {
    int bad = 0;
    const u32 B = BTB_GAS_BLOCK;
    const std::vector<u32> edges = {0, 1, 15, 16, 17, 31, 33, 63, 64, 65, B - 1, B, B + 1, 3 * B + 1, 0, 5};
    for (u32 mis : {0u, 1u, 3u, 7u, 8u, 9u, 15u}) {
        bad += run(edges, mis, 3, 2, true);
        for (u32 n : {1u, 15u, 16u, 17u, B - 1, B, B + 1, 2 * B, 3 * B + 1}) bad += run({n}, mis, 0, 0, false);
        bad += run({0, 0, 2000, 0, 0}, mis, 0, 0, false);
        bad += run({700, 700}, mis, 0, 0, false, nullptr, 0);     // all-zero calldata
        bad += run({700, 700}, mis, 0, 0, false, nullptr, 0xff);  // zero-free
        bad += run({3, 4, 5, 6, 7, 8, 9, 1, 2, 3, 4, 5, 6, 7, 8, 9}, mis, 0, 0, false);
    }
    bad += run({}, 0, 0, 0, false);
    bad += run({0, 0, 0}, 0, 0, 65, true);
    for (u64 h : {0ull, 1ull, 255ull, 256ull}) bad += run({}, 0, h, 1, true);
    u64 cross[4];
    memcpy(cross, BTB_P64, 32);
    cross[0] += 3;  // number = p + 3: number - 8 + j crosses p at j = 5
    bad += run({}, 0, 8, 0, true, cross);
    const u64 top[4] = {~0ull, ~0ull, ~0ull, ~0ull};
    bad += run({}, 0, 5, 0, true, top);
    printf("block_tables_asan: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
