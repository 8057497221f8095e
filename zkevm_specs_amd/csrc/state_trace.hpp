// State circuit from compact trace records (zk_state_verify_from_trace*, zk_state_ops_from_trace*): the records zk_evm_witness_from_trace
// expands into 448-byte wire rows (trace_witness.hpp) are a third provider of the cells the RW -> State re-keying (state_rekey.hpp) and the
// fused State pass (state_fused.hpp) read, beside the op list and the wire rows.
//
// The results are DEFINED BY COMPOSITION: bit for bit those of the matching _from_rw entry over the rw / rw_flags zk_evm_witness_from_trace
// writes for the same records.  So a cell here is trw_rw_piece's cell, reductions included: a pool address is FQ(w), a wide value without
// its is_word bit (w mod p, 0), with it (w mod 2^128, w >> 128), an absent key / aux0 Word(0).  The State circuit reads rw_counter,
// is_write, tag, id, address, field_tag, storage_key, value and aux0: cells 0..9, 12, 13.  value_prev (cells 10, 11) is never read, so
// `prev` may be null and these functions do not provide it.
//
//   StrcRec / strc_load      the six scalars of a record (head, counter, id, addr, val, pool offset), each loaded once
//   StrcRow / strc_load_row  + the row's pool words (address, key, value, aux0), each loaded once behind its head bit
//   strc_row_cell            cell k of a loaded row: arithmetic only
//   strc_cell                cell k of row `row` on its own (loads what that cell needs; hostsim, CPU backend, definition)
//   strc_stream_*            the SORTED PACKED OP STREAM of the verdict session: op j's six scalars as one 48-byte record in State order,
//                            written once by the first pass; wide cells stay in the pool and are reached through the stored offset
// k_state_trace.hip maps lanes onto these; cpu_backend.cpp runs them in host loops.
#pragma once
#include "trace_witness.hpp"
#include "state_assign.hpp"
#if !defined(ZK_HOSTSIM)
#include "state_fused.hpp"
#endif

struct StrcArgs {
    const u32* head;   // [n] the session's copy of the checked heads
    const u64* ctr;    // [n] the session's copy of the checked counters (null: rw_base + i)
    const u64* id;     // [n]
    const u64* addr;   // [n]
    const u64* val;    // [n]
    const u64* off;    // [n] pool words consumed by the rows before row i (trw_offset_scan_kernel)
    const u64* pool;   // [n_pool][4]
    u64 n, rw_base;
    u64* stream;       // [n_ops][STRC_STREAM_WORDS] the sorted packed op stream (verdict session; null otherwise)
};
enum { STRC_STREAM_WORDS = 6 };  // head, counter, id, addr, val, pool offset: 48 bytes

struct StrcRec {
    u32 head;
    u64 ctr, id, addr, val, off;
};
struct StrcRow {
    StrcRec r;
    Fr w_addr, w_key, w_val, w_aux;  // the row's pool words (zero where the head names none)
};

ZK_HD StrcRec strc_load(const StrcArgs& a, u64 row) {
    StrcRec r;
    r.head = a.head[row];
    r.ctr = a.ctr ? a.ctr[row] : a.rw_base + row;
    r.id = a.id[row];
    r.addr = a.addr[row];
    r.val = a.val[row];
    r.off = a.off[row];
    return r;
}
// positions of the row's pool words (order: address, key, value, prev, aux)
ZK_HD u64 strc_p_key(u32 h, u64 off) { return off + ((h >> 20) & 1u); }
ZK_HD u64 strc_p_val(u32 h, u64 off) { return strc_p_key(h, off) + ((h >> 21) & 1u); }
ZK_HD u64 strc_p_aux(u32 h, u64 off) { return strc_p_val(h, off) + ((h >> 22) & 1u) + ((h >> 23) & 1u); }
// the four loads are independent of each other and of what the cells then select; rows without pool words (most) issue none
ZK_HD StrcRow strc_widen(const u64* pool, const StrcRec& r) {
    StrcRow R;
    R.r = r;
    const u32 h = r.head;
    R.w_addr = (h & TRW_H_ADDR_POOL) ? fr_load(pool + 4 * r.off) : fr_zero();
    R.w_key = (h & TRW_H_KEY) ? fr_load(pool + 4 * strc_p_key(h, r.off)) : fr_zero();
    R.w_val = (h & TRW_H_VALUE_POOL) ? fr_load(pool + 4 * strc_p_val(h, r.off)) : fr_zero();
    R.w_aux = (h & TRW_H_AUX) ? fr_load(pool + 4 * strc_p_aux(h, r.off)) : fr_zero();
    return R;
}
ZK_HD StrcRow strc_load_row(const StrcArgs& a, u64 row) { return strc_widen(a.pool, strc_load(a, row)); }

// Cell k (0..9, 12, 13) of the wire row of a loaded record.
ZK_HD Fr strc_row_cell(const StrcRow& R, u32 k) {
    const u32 h = R.r.head;
    switch (k) {
    case 0: return fr_from_u64(R.r.ctr);
    case 1: return fr_from_u64(h & 1u);
    case 2: return fr_from_u64((h >> TRW_H_TAG_SHIFT) & 0xfu);
    case 3: return fr_from_u64(R.r.id);
    case 4: return (h & TRW_H_ADDR_POOL) ? btb_reduce(R.w_addr) : fr_from_u64(R.r.addr);
    case 5: return fr_from_u64((h >> TRW_H_FIELD_SHIFT) & 0xffu);
    case 6: return u256_lo(R.w_key);  // (zero when absent)
    case 7: return u256_hi(R.w_key);
    case 8:
        if (!(h & TRW_H_VALUE_POOL)) return fr_from_u64(R.r.val);
        return (h & TRW_H_VALUE_WORD) ? u256_lo(R.w_val) : btb_reduce(R.w_val);
    case 9: return ((h & TRW_H_VALUE_POOL) && (h & TRW_H_VALUE_WORD)) ? u256_hi(R.w_val) : fr_zero();
    case 12: return u256_lo(R.w_aux);
    case 13: return u256_hi(R.w_aux);
    default: return fr_zero();
    }
}
// Cell k of row `row` on its own, by trw_rw_piece's rules: the cell selects what to load — an immediate from the head, one 64-bit
// integer, one half of a pool word, or a pool word to reduce — and the one load stands behind the selection.
ZK_HD Fr strc_cell(const StrcArgs& a, u64 row, u32 h, u64 off, u32 k) {
    u64 imm = 0;
    const u64* one = nullptr;   // the cell is *one
    const u64* half = nullptr;  // the cell is the 128 bits at half[0..1]
    const u64* red = nullptr;   // the cell is FQ(red[0..3])
    switch (k) {
    case 0: if (a.ctr) one = a.ctr + row; else imm = a.rw_base + row; break;
    case 1: imm = h & 1u; break;
    case 2: imm = (h >> TRW_H_TAG_SHIFT) & 0xfu; break;
    case 3: one = a.id + row; break;
    case 4: if (h & TRW_H_ADDR_POOL) red = a.pool + 4 * off; else one = a.addr + row; break;
    case 5: imm = (h >> TRW_H_FIELD_SHIFT) & 0xffu; break;
    case 6: case 7: if (h & TRW_H_KEY) half = a.pool + 4 * strc_p_key(h, off) + (k == 7 ? 2 : 0); break;
    case 8: case 9: {
        const u64* w = a.pool + 4 * strc_p_val(h, off);  // (dereferenced only when wide)
        if (!(h & TRW_H_VALUE_POOL)) { if (k == 8) one = a.val + row; }
        else if (h & TRW_H_VALUE_WORD) half = w + (k == 9 ? 2 : 0);
        else if (k == 8) red = w;
        break;
    }
    case 12: case 13: if (h & TRW_H_AUX) half = a.pool + 4 * strc_p_aux(h, off) + (k == 13 ? 2 : 0); break;
    default: break;
    }
    if (red) return btb_reduce(fr_load(red));
    Fr r = fr_from_u64(one ? *one : imm);
    if (half) {
        r.v[0] = (u32)half[0]; r.v[1] = (u32)(half[0] >> 32);
        r.v[2] = (u32)half[1]; r.v[3] = (u32)(half[1] >> 32);
    }
    return r;
}

// ---- the re-keying over a loaded row ---------------------------------------------------------------------------------------------------
ZK_HD RwkKey strc_key(const StrcRow& R) {
    return rwk_key_of([&R](int k) { return strc_row_cell(R, (u32)k); });
}
ZK_HD RwkOp strc_op(const StrcRow& R, const RwkKey& k) {
    return rwk_op_of([&R](int c) { return strc_row_cell(R, (u32)c); }, trw_rw_flag(R.r.head), k);
}

// ---- the sorted packed op stream (verdict session) ---------------------------------------------------------------------------------------
// Op 0 is the StartOp: a record with tag nibble 1 (Target.Start -> Tag.Start) and zeros re-keys to rwk_emit_start's op in every slot but
// lexicographic_ordering_selector, which strc_row_slot answers from the op index.
ZK_HD void strc_stream_store(u64* stream, u64 j, const StrcRec& r) {
    u64* p = stream + j * STRC_STREAM_WORDS;
#if defined(ZK_HOSTSIM)
    p[0] = r.head; p[1] = r.ctr; p[2] = r.id; p[3] = r.addr; p[4] = r.val; p[5] = r.off;
#else
    uint4* q = (uint4*)p;  // 48-byte records: 16-byte aligned
    q[0] = make_uint4(r.head, 0u, (u32)r.ctr, (u32)(r.ctr >> 32));
    q[1] = make_uint4((u32)r.id, (u32)(r.id >> 32), (u32)r.addr, (u32)(r.addr >> 32));
    q[2] = make_uint4((u32)r.val, (u32)(r.val >> 32), (u32)r.off, (u32)(r.off >> 32));
#endif
}
ZK_HD StrcRec strc_stream_start() {
    StrcRec r;
    r.head = 1u << TRW_H_TAG_SHIFT;
    r.ctr = r.id = r.addr = r.val = r.off = 0;
    return r;
}
ZK_HD StrcRec strc_stream_load(const u64* stream, u64 j) {
    const u64* p = stream + j * STRC_STREAM_WORDS;
    StrcRec r;
#if defined(ZK_HOSTSIM)
    r.head = (u32)p[0]; r.ctr = p[1]; r.id = p[2]; r.addr = p[3]; r.val = p[4]; r.off = p[5];
#else
    const uint4* q = (const uint4*)p;
    const uint4 a = q[0], b = q[1], c = q[2];
    r.head = a.x;
    r.ctr = (u64)a.z | ((u64)a.w << 32);
    r.id = (u64)b.x | ((u64)b.y << 32);
    r.addr = (u64)b.z | ((u64)b.w << 32);
    r.val = (u64)c.x | ((u64)c.y << 32);
    r.off = (u64)c.z | ((u64)c.w << 32);
#endif
    return r;
}
ZK_HD StrcRow strc_stream_row(const StrcArgs& a, u64 j) { return strc_widen(a.pool, strc_stream_load(a.stream, j)); }
// slot s of op j of the stream, from its loaded row (asg_slot_of_rw_row over the record's cells)
ZK_HD Fr strc_row_slot(const StrcRow& R, u32 s, bool start) {
    if (s == ASG_LEX) return fr_from_u64(start ? 0 : 1);
    return asg_slot_of_rw_row([&R](int k) { return strc_row_cell(R, (u32)k); }, s);
}
ZK_HD u32 strc_row_flags(const StrcRow& R, bool start) {  // asg_flags<true>
    if (start) return 0u;
    const u32 tag = rwk_tag_of_target((R.r.head >> TRW_H_TAG_SHIFT) & 0xfu);
    return (trw_rw_flag(R.r.head) & 1u) | ((tag == 4u || tag == 6u) ? 2u : 0u) | (tag == 6u ? 4u : 0u);
}
ZK_HD AsgKey strc_mpt_key(const StrcArgs& a, u64 j) {
    const StrcRow R = strc_stream_row(a, j);
    AsgKey k;
    k.addr = asg_reduce(strc_row_slot(R, ASG_ADDR, j == 0));
    k.ft = asg_reduce(strc_row_slot(R, ASG_FT, j == 0));
    k.key = strc_row_slot(R, ASG_KEY, j == 0);
    return k;
}
ZK_HD bool strc_stream_has_key(const StrcArgs& a, u64 j) {  // asg_has_key of the op's tag: Storage (4) / Account (6)
    const u32 tag = rwk_tag_of_target(((u32)a.stream[j * STRC_STREAM_WORDS] >> TRW_H_TAG_SHIFT) & 0xfu);
    return j != 0 && (tag == 4u || tag == 6u);
}

#if !defined(ZK_HOSTSIM)
// ---- the fused State pass over the stream (device) ---------------------------------------------------------------------------------------------
struct StateTraceArgs : StateArgs {
    AssignArgs asg;
    StrcArgs src;
};
ZK_HD void state_row_from_stream(const StateTraceArgs& a, u64 i, StRow& R, u32& code, u32& asg_code) {
    const AssignArgs& g = a.asg;
    const u32 root_rank = g.root_rank[i];
    const bool is_first = g.first[i] == (u32)i;
    const bool start = i == 0;
    const StrcRow row = strc_stream_row(a.src, i);
    state_row_from_slots([&row, start](u32 s) { return strc_row_slot(row, s, start); }, strc_row_flags(row, start), is_first, root_rank, R, code, asg_code);
}
ZK_HD Fr st_src_lex(const StateTraceArgs& a, u64 i) { return fr_from_u64(i == 0 ? 0 : 1); }
ZK_HD u32 st_src_next_keys_diff(const StateTraceArgs& a, u64 j, const Fr* const mine[6]) {
    const StrcRow row = strc_stream_row(a.src, j);
    const bool start = j == 0;
    const Fr key = strc_row_slot(row, ASG_KEY, start);
    const Fr c[6] = {asg_reduce(strc_row_slot(row, ASG_TAG, start)), asg_reduce(strc_row_slot(row, ASG_ID, start)), asg_reduce(strc_row_slot(row, ASG_ADDR, start)),
                     asg_reduce(strc_row_slot(row, ASG_FT, start)), u256_lo(key), u256_hi(key)};
    u32 d = 0;
#pragma unroll
    for (int x = 0; x < 6; x++)
#pragma unroll
        for (int k = 0; k < 8; k++) d |= c[x].v[k] ^ mine[x]->v[k];
    return d;
}
#endif
