// Stand-alone host program (TEST INFRASTRUCTURE): the per-element functions of csrc/bytecode_code.hpp over exactly-sized heap buffers,
// built with -fsanitize=address,undefined by tests/test_bytecode_from_code_cpu.py and run as a child process.  Shapes: code lengths at
// the 64-byte chunk edges, several codes per call, empty codes, and circuits cut at, one before and one after 2^k rows.  Every table
// row is compared with the byte-by-byte recurrence; exit status 0 = no mismatch (the sanitizers abort on their own findings).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../zkevm_specs_amd/csrc/bytecode_code.hpp"

static u64 cell_lo(const u64* p) { return p[0]; }
static bool cell_small(const u64* p) { return !p[1] && !p[2] && !p[3]; }

static int run(const std::vector<std::vector<uint8_t>>& codes, u32 k) {
    const u64 n_codes = codes.size();
    std::vector<u64> off(n_codes + 1, 0);
    for (u64 j = 0; j < n_codes; j++) off[j + 1] = off[j] + codes[j].size();
    const u64 n_bytes = off[n_codes], n_rows = n_bytes + n_codes, n_out = k ? 1ull << k : 0;
    // (the sponge reads whole aligned 64-bit words: the byte buffer is sized to the next word, as the backends stage it)
    std::vector<uint8_t> code((n_bytes + 15) & ~7ull, 0);
    for (u64 j = 0; j < n_codes; j++)
        if (!codes[j].empty()) memcpy(code.data() + off[j], codes[j].data(), codes[j].size());
    std::vector<BcaChunk> chunks;
    std::vector<u32> row_off(n_codes + 1), chunk0(n_codes + 1);
    for (u64 j = 0; j < n_codes; j++) {
        row_off[j] = (u32)(off[j] + j);
        chunk0[j] = (u32)chunks.size();
        for (u64 b = off[j]; b < off[j + 1]; b += BCA_CHUNK) {
            BcaChunk c;
            c.code = (u32)j; c.start = (u32)b; c.first = 0;
            c.count = (u32)(off[j + 1] - b < BCA_CHUNK ? off[j + 1] - b : BCA_CHUNK);
            chunks.push_back(c);
        }
    }
    row_off[n_codes] = (u32)n_rows;
    chunk0[n_codes] = (u32)chunks.size();
    const u64 nc = chunks.size();
    u64 rand[4] = {0x1234567890abcdefull, 0x0fedcba987654321ull, 0x1111111122222222ull, 0x0123456789abcdefull};
    std::vector<u64> rpow(BCA_RPOW_ROWS * 4), krpow(KT_RPOW_ROWS * 4), acc(nc * 4), cin(nc * 4), part(n_bytes * 4), krows(n_codes * KT_NCELLS * 4),
        table(n_rows * BCC_TABLE_NCELLS * 4), rows(n_out * BCA_OUT_NCELLS * 4);
    std::vector<u32> cm(nc), cstate(nc);
    std::vector<uint8_t> cmap(nc * BCA_MAP_STRIDE);
    bca_fill_rpow(fr_load(rand), rpow.data());
    kt_fill_rpow(fr_load(rand), krpow.data());
    KeccakGenArgs g;
    g.data = code.data(); g.offsets = off.data(); g.n = n_codes; g.rpow = krpow.data(); g.rows = krows.data(); g.mode = KT_MODE_CIRCUIT;
    g.long_list = nullptr; g.long_count = nullptr;
    BccArgs a;
    memset(&a, 0, sizeof a);
    a.code = code.data(); a.offsets = off.data(); a.row_off = row_off.data();
    a.n_bytes = n_bytes; a.n_codes = n_codes; a.n_rows = n_rows; a.n_out = n_out;
    a.p.chunks = chunks.data(); a.p.code_chunk0 = chunk0.data(); a.p.n_chunks = nc; a.p.n_codes = n_codes; a.p.rpow = rpow.data();
    a.p.chunk_acc = acc.data(); a.p.chunk_in = cin.data(); a.p.chunk_m = cm.data(); a.p.chunk_state = cstate.data(); a.p.chunk_map = cmap.data();
    a.part = part.data(); a.keccak = krows.data(); a.table = table.data(); a.rows = rows.data();
    for (u64 c = 0; c < nc; c++) bcc_chunk(a, c);
    for (u64 j = 0; j < n_codes; j++) bca_prefix_code(a.p, j);
    for (u64 j = 0; j < n_codes; j++) keccak_table_row(g, j);
    const u64 lanes = n_rows > n_out ? n_rows : n_out;
    for (u64 i = 0; i < lanes; i++) bcc_write_row(a, i);
    // the table against the byte-by-byte recurrence
    int bad = 0;
    u64 i = 0;
    for (u64 j = 0; j < n_codes; j++) {
        const u64* h = table.data() + i * 24;
        bad += !(cell_lo(h + 8) == 1 && cell_lo(h + 12) == 0 && cell_lo(h + 16) == 0 && cell_lo(h + 20) == codes[j].size());
        bad += memcmp(h, krows.data() + (j * KT_NCELLS + 3) * 4, 64) != 0;
        i++;
        u32 left = 0;
        for (u64 q = 0; q < codes[j].size(); q++, i++) {
            const u64* t = table.data() + i * 24;
            const u32 b = codes[j][q];
            bad += !(cell_lo(t + 8) == 2 && cell_lo(t + 12) == q && cell_lo(t + 16) == (left == 0 ? 1u : 0u) && cell_lo(t + 20) == b);
            bad += !(cell_small(t + 8) && cell_small(t + 12) && cell_small(t + 16) && cell_small(t + 20));
            bad += memcmp(t, h, 64) != 0;
            if (i < n_out) bad += cell_lo(rows.data() + (8 * n_out + i) * 4) != left;
            left = left == 0 ? bcc_push_size(b) : left - 1;
        }
    }
    for (u64 r = n_rows; r < n_out; r++) bad += !(cell_lo(rows.data() + (4 * n_out + r) * 4) == 1 && cell_lo(rows.data() + (10 * n_out + r) * 4) == 0);
    if (n_out) bad += !(cell_lo(rows.data()) == 1 && cell_lo(rows.data() + (1 * n_out + n_out - 1) * 4) == 1);
    if (bad) fprintf(stderr, "bytecode_code_asan: %d mismatches (%llu codes, k = %u)\n", bad, (unsigned long long)n_codes, k);
    return bad;
}

static std::vector<uint8_t> make(u32 n, u32 seed) {
    std::vector<uint8_t> c(n);
    u32 x = seed * 2654435761u + 12345u;
    for (u32 q = 0; q < n; q++) {
        x = x * 1664525u + 1013904223u;
        const u32 v = x >> 24;
        c[q] = (uint8_t)((x >> 9) % 10u < 3u ? 0x60u + (v & 31u) : v);  // 30 % PUSH1..PUSH32
    }
    return c;
}

int main() {
    int bad = 0;
    const u32 edges[] = {0, 1, 31, 32, 33, 34, 62, 63, 64, 65, 66, 126, 127, 128, 129, 130, 135, 136, 137, 271, 272, 273};
    std::vector<std::vector<uint8_t>> all;
    for (u32 n : edges) {
        bad += run({make(n, n)}, 10);  // one code per call
        bad += run({make(n, n + 7)}, 0);
        all.push_back(make(n, n + 99));
    }
    bad += run(all, 12);  // every edge length in one call
    bad += run(all, 0);
    bad += run({}, 3);
    bad += run({}, 0);
    bad += run({std::vector<uint8_t>(), std::vector<uint8_t>(), make(5, 1), std::vector<uint8_t>()}, 4);
    // 2^k - 1, 2^k, 2^k + 1 rows (k = 8) with a PUSH32 whose data runs over the cut; a cut inside a later code; k = 1
    for (u32 total : {255u, 256u, 257u}) {
        std::vector<uint8_t> c(total - 1, 0);
        c[240] = 0x7f;
        for (u32 q = 241; q < total - 1; q++) c[q] = 0x61;
        bad += run({c}, 8);
    }
    std::vector<uint8_t> second(200, 0);
    second[140] = 0x7f;
    for (u32 q = 141; q < 173; q++) second[q] = 0x62;
    bad += run({make(100, 3), second, make(50, 4)}, 8);
    bad += run({make(100, 3), second, make(50, 4)}, 1);
    std::vector<std::vector<uint8_t>> cross;
    for (u32 j = 0; j < 64; j++) {
        std::vector<uint8_t> c(j + 1 + 200, 0x60);
        for (u32 q = 0; q < j; q++) c[q] = 0;
        c[j] = 0x7f;
        cross.push_back(c);
    }
    bad += run(cross, 15);
    printf("bytecode_code_asan: %s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
