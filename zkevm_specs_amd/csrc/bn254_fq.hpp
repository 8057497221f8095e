// BN254 (alt_bn128, EIP-196 / EIP-197) base field Fq, its tower Fq2 / Fq6 / Fq12, the curve and its twist, and the optimal-ate
// pairing, for the ECC circuit (ecc_circuit.hpp).
//
// Fq is p = 21888242871839275222246405745257275088696311157297823662689037894645226208583 in 8 x u32 limbs, Montgomery form with
// R = 2^256 (CIOS as fr.hpp).  Unlike the circuit cells of fr.hpp, every Fq value here stays in Montgomery form from load to the
// final comparison: the curve / pairing chains are long and no intermediate is compared with a witness cell.
//   Fq2  = Fq[u] / (u^2 + 1)
//   Fq6  = Fq2[v] / (v^3 - xi),  xi = 9 + u
//   Fq12 = Fq6[w] / (w^2 - v)
// The twist is the D-type sextic twist E': y^2 = x^3 + 3 / xi over Fq2 (EIP-197's G2), untwisted by (x, y) -> (x w^2, y w^3).
//
// The curve code is written once over a field type F (Fq for G1, Fq2 for G2).  Two forms of scalar multiplication exist:
//   * the exact replay of py_ecc's affine chain (`multiply` / `double` / `add` of bn128_curve.py, inverse(0) = 0), which is what the
//     reference computes also for points that are not on the curve;
//   * a Jacobian chain that agrees with it whenever the affine chain meets no zero denominator (see jac_mul_checked).
// Constants: bn254_constants.h (gen_bn254_constants.py).
#pragma once
#include "fr.hpp"
#include "bn254_constants.h"

namespace bn {

struct Fq {
    u32 v[8];
};
struct Fq2 {
    Fq c0, c1;
};
struct Fq6 {
    Fq2 c0, c1, c2;
};
struct Fq12 {
    Fq6 c0, c1;
};

#define BN_FQ_CONST(name, limbs) ZK_HD Fq name() { Fq r = {limbs}; return r; }
BN_FQ_CONST(fq_modulus, FQ_P_LIMBS)
BN_FQ_CONST(fq_one, FQ_ONE_LIMBS)
BN_FQ_CONST(fq_r2, FQ_R2_LIMBS)
BN_FQ_CONST(fq_b, FQ_B_M_LIMBS)
BN_FQ_CONST(fq_inv_neg2, FQ_INV_NEG2_M_LIMBS)

ZK_HD Fq fq_zero() {
    Fq r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = 0;
    return r;
}
ZK_HD Fq fq_load_raw(const u64* p) {  // a 256-bit word, as it is (the caller reduces)
    Fq r;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        r.v[2 * i] = (u32)p[i];
        r.v[2 * i + 1] = (u32)(p[i] >> 32);
    }
    return r;
}
ZK_HD void fq_store_raw(const Fq& a, u64* p) {
#pragma unroll
    for (int i = 0; i < 4; i++) p[i] = (u64)a.v[2 * i] | ((u64)a.v[2 * i + 1] << 32);
}
ZK_HD bool fq_is_zero(const Fq& a) {
    u32 o = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) o |= a.v[i];
    return o == 0;
}
ZK_HD bool fq_eq(const Fq& a, const Fq& b) {
    u32 o = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) o |= a.v[i] ^ b.v[i];
    return o == 0;
}
ZK_HD u32 fq_sub_raw(Fq& r, const Fq& a, const Fq& b) {
    u64 bw = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        u64 t = (u64)a.v[i] - b.v[i] - bw;
        r.v[i] = (u32)t;
        bw = (t >> 32) & 1;
    }
    return (u32)bw;
}
ZK_HD u32 fq_add_raw(Fq& r, const Fq& a, const Fq& b) {
    u64 c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        c += (u64)a.v[i] + b.v[i];
        r.v[i] = (u32)c;
        c >>= 32;
    }
    return (u32)c;
}
ZK_HD bool fq_lt_p(const Fq& a) {  // a < p as integers (a 256-bit word)
    Fq t;
    return fq_sub_raw(t, a, fq_modulus()) != 0;
}
// FP(x) of the reference (int -> residue mod p) for any 256-bit x: 2^256 < 6p, at most five subtractions
ZK_HD Fq fq_reduce(const Fq& a) {
    Fq r = a;
    for (int k = 0; k < 5; k++) {
        Fq t;
        if (fq_sub_raw(t, r, fq_modulus())) break;
        r = t;
    }
    return r;
}
ZK_HD Fq fq_add(const Fq& a, const Fq& b) {
    Fq s, t;
    fq_add_raw(s, a, b);  // a, b < p < 2^254: no carry out
    return fq_sub_raw(t, s, fq_modulus()) ? s : t;
}
ZK_HD Fq fq_sub(const Fq& a, const Fq& b) {
    Fq d, t;
    const u32 bw = fq_sub_raw(d, a, b);
    fq_add_raw(t, d, fq_modulus());
    return bw ? t : d;
}
ZK_HD Fq fq_neg(const Fq& a) { return fq_sub(fq_zero(), a); }
ZK_HD Fq fq_dbl(const Fq& a) { return fq_add(a, a); }

// Montgomery product a * b * R^-1 mod p (CIOS on 8 x 32-bit limbs); inputs < p.
ZK_NOINLINE Fq fq_mont(Fq a, Fq b) {
    const Fq p = fq_modulus();
    u32 t[10];
#pragma unroll
    for (int i = 0; i < 10; i++) t[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        u64 c = 0;
        const u32 bi = b.v[i];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            c += (u64)a.v[j] * bi + t[j];
            t[j] = (u32)c;
            c >>= 32;
        }
        c += t[8];
        t[8] = (u32)c;
        t[9] = (u32)(c >> 32);
        const u32 m = t[0] * FQ_INV32;
        c = (u64)m * p.v[0] + t[0];
        c >>= 32;
#pragma unroll
        for (int j = 1; j < 8; j++) {
            c += (u64)m * p.v[j] + t[j];
            t[j - 1] = (u32)c;
            c >>= 32;
        }
        c += t[8];
        t[7] = (u32)c;
        t[8] = t[9] + (u32)(c >> 32);
    }
    Fq r, s;
#pragma unroll
    for (int i = 0; i < 8; i++) r.v[i] = t[i];
    const u32 bw = fq_sub_raw(s, r, p);
    return (t[8] || !bw) ? s : r;
}
ZK_HD Fq fq_to_mont(const Fq& a) { return fq_mont(a, fq_r2()); }  // a < p
ZK_HD Fq fq_from_mont(const Fq& a) {
    Fq one = fq_zero();
    one.v[0] = 1u;
    return fq_mont(a, one);
}
// bit k of a 256-bit integer; the limb is selected with static indices (a dynamic index would put the limbs in scratch memory)
ZK_HD u32 fq_bit(const Fq& n, int k) {
    u32 w = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) w = (i == (k >> 5)) ? n.v[i] : w;
    return (w >> (k & 31)) & 1u;
}
// a^(p - 2): py_ecc's prime_field_inv, which returns 0 for 0
ZK_HD Fq fq_inv(const Fq& a) {
    const Fq e = {FQ_PM2_LIMBS};
    Fq acc = a;  // bit 253 of p - 2 is its top bit
    for (int bit = 252; bit >= 0; bit--) {
        acc = fq_mont(acc, acc);
        if (fq_bit(e, bit)) acc = fq_mont(acc, a);
    }
    return acc;
}

// ---- the field interface the curve templates use (Fq and Fq2 overloads) ----------------------------------------------------
ZK_HD Fq f_add(const Fq& a, const Fq& b) { return fq_add(a, b); }
ZK_HD Fq f_sub(const Fq& a, const Fq& b) { return fq_sub(a, b); }
ZK_HD Fq f_neg(const Fq& a) { return fq_neg(a); }
ZK_HD Fq f_mul(const Fq& a, const Fq& b) { return fq_mont(a, b); }
ZK_HD Fq f_sqr(const Fq& a) { return fq_mont(a, a); }
ZK_HD Fq f_inv(const Fq& a) { return fq_inv(a); }
ZK_HD bool f_is_zero(const Fq& a) { return fq_is_zero(a); }
ZK_HD bool f_eq(const Fq& a, const Fq& b) { return fq_eq(a, b); }
ZK_HD Fq f_mul_base(const Fq& a, const Fq& k) { return fq_mont(a, k); }  // by an Fq scalar
ZK_HD void f_zero(Fq& a) { a = fq_zero(); }
ZK_HD void f_one(Fq& a) { a = fq_one(); }

ZK_HD Fq2 fq2_make(const Fq& a, const Fq& b) {
    Fq2 r;
    r.c0 = a;
    r.c1 = b;
    return r;
}
ZK_HD Fq2 f_add(const Fq2& a, const Fq2& b) { return fq2_make(fq_add(a.c0, b.c0), fq_add(a.c1, b.c1)); }
ZK_HD Fq2 f_sub(const Fq2& a, const Fq2& b) { return fq2_make(fq_sub(a.c0, b.c0), fq_sub(a.c1, b.c1)); }
ZK_HD Fq2 f_neg(const Fq2& a) { return fq2_make(fq_neg(a.c0), fq_neg(a.c1)); }
ZK_HD Fq2 f_mul(const Fq2& a, const Fq2& b) {  // Karatsuba, u^2 = -1
    const Fq t0 = fq_mont(a.c0, b.c0), t1 = fq_mont(a.c1, b.c1);
    const Fq t2 = fq_mont(fq_add(a.c0, a.c1), fq_add(b.c0, b.c1));
    return fq2_make(fq_sub(t0, t1), fq_sub(fq_sub(t2, t0), t1));
}
ZK_HD Fq2 f_sqr(const Fq2& a) {  // (a0 + a1)(a0 - a1) + 2 a0 a1 u
    const Fq t = fq_mont(a.c0, a.c1);
    return fq2_make(fq_mont(fq_add(a.c0, a.c1), fq_sub(a.c0, a.c1)), fq_dbl(t));
}
ZK_HD Fq2 f_inv(const Fq2& a) {  // conj(a) / (a0^2 + a1^2); 0 -> 0 as py_ecc's FQP.inv
    const Fq d = fq_inv(fq_add(fq_mont(a.c0, a.c0), fq_mont(a.c1, a.c1)));
    return fq2_make(fq_mont(a.c0, d), fq_neg(fq_mont(a.c1, d)));
}
ZK_HD bool f_is_zero(const Fq2& a) { return fq_is_zero(a.c0) && fq_is_zero(a.c1); }
ZK_HD bool f_eq(const Fq2& a, const Fq2& b) { return fq_eq(a.c0, b.c0) && fq_eq(a.c1, b.c1); }
ZK_HD Fq2 f_mul_base(const Fq2& a, const Fq& k) { return fq2_make(fq_mont(a.c0, k), fq_mont(a.c1, k)); }
ZK_HD void f_zero(Fq2& a) { a.c0 = fq_zero(); a.c1 = fq_zero(); }
ZK_HD void f_one(Fq2& a) { a.c0 = fq_one(); a.c1 = fq_zero(); }
ZK_HD Fq2 fq2_conj(const Fq2& a) { return fq2_make(a.c0, fq_neg(a.c1)); }
ZK_HD Fq2 fq2_mul_xi(const Fq2& a) {  // (a0 + a1 u)(9 + u) = 9 a0 - a1 + (a0 + 9 a1) u
    Fq a0_9 = fq_dbl(fq_dbl(fq_dbl(a.c0)));
    a0_9 = fq_add(a0_9, a.c0);
    Fq a1_9 = fq_dbl(fq_dbl(fq_dbl(a.c1)));
    a1_9 = fq_add(a1_9, a.c1);
    return fq2_make(fq_sub(a0_9, a.c1), fq_add(a.c0, a1_9));
}
ZK_HD Fq2 fq2_twist_b() {
    const Fq2 r = FQ2_TWIST_B_M;
    return r;
}
ZK_HD Fq curve_b(const Fq&) { return fq_b(); }
ZK_HD Fq2 curve_b(const Fq2&) { return fq2_twist_b(); }

// ---- curve points over F ------------------------------------------------------------------------------------------------------
template <class F> struct Aff {  // py_ecc's affine point; inf = its None
    F x, y;
    bool inf;
};
template <class F> struct Jac {  // X / Z^2, Y / Z^3; Z = 0 is the point at infinity
    F X, Y, Z;
};

template <class F> ZK_HD bool on_curve(const Aff<F>& a) {  // is_on_curve(pt, b): None is on every curve
    if (a.inf) return true;
    return f_eq(f_sub(f_sqr(a.y), f_mul(f_sqr(a.x), a.x)), curve_b(a.x));
}
// py_ecc's double(pt): m = 3x^2 / 2y (inverse(0) = 0, so a point (x, 0) doubles to (-2x, 0))
template <class F> ZK_HD Aff<F> aff_double(const Aff<F>& a) {
    if (a.inf) return a;
    const F x2 = f_sqr(a.x);
    const F m = f_mul(f_add(f_add(x2, x2), x2), f_inv(f_add(a.y, a.y)));
    Aff<F> r;
    r.inf = false;
    r.x = f_sub(f_sqr(m), f_add(a.x, a.x));
    r.y = f_sub(f_mul(m, f_sub(a.x, r.x)), a.y);  // -m newx + m x - y
    return r;
}
// py_ecc's add(p1, p2)
template <class F> ZK_HD Aff<F> aff_add(const Aff<F>& a, const Aff<F>& b) {
    if (a.inf || b.inf) return b.inf ? a : b;
    if (f_eq(a.x, b.x)) {
        if (f_eq(a.y, b.y)) return aff_double(a);
        Aff<F> r = a;
        r.inf = true;
        return r;
    }
    const F m = f_mul(f_sub(b.y, a.y), f_inv(f_sub(b.x, a.x)));
    Aff<F> r;
    r.inf = false;
    r.x = f_sub(f_sub(f_sqr(m), a.x), b.x);
    r.y = f_sub(f_mul(m, f_sub(a.x, r.x)), a.y);
    return r;
}

template <class F> ZK_HD Jac<F> jac_from_aff(const Aff<F>& a) {
    Jac<F> r;
    r.X = a.x;
    r.Y = a.y;
    f_one(r.Z);
    if (a.inf) f_zero(r.Z);
    return r;
}
template <class F> ZK_HD bool jac_is_inf(const Jac<F>& a) { return f_is_zero(a.Z); }
// dbl-2009-l (a = 0); Y = 0 gives Z = 0, the group law's answer (the affine formula's differs: the callers detect that case)
template <class F> ZK_HD Jac<F> jac_double(const Jac<F>& p) {
    const F A = f_sqr(p.X), B = f_sqr(p.Y), C = f_sqr(B);
    F D = f_sub(f_sub(f_sqr(f_add(p.X, B)), A), C);
    D = f_add(D, D);
    const F E = f_add(f_add(A, A), A);
    const F Fv = f_sqr(E);
    Jac<F> r;
    r.X = f_sub(Fv, f_add(D, D));
    F C8 = f_add(C, C);
    C8 = f_add(C8, C8);
    C8 = f_add(C8, C8);
    r.Y = f_sub(f_mul(E, f_sub(D, r.X)), C8);
    const F YZ = f_mul(p.Y, p.Z);
    r.Z = f_add(YZ, YZ);
    return r;
}
// add-2007-bl with the exceptional cases (equal points double, opposite points give infinity)
template <class F> ZK_HD Jac<F> jac_add(const Jac<F>& p, const Jac<F>& q) {
    if (jac_is_inf(p)) return q;
    if (jac_is_inf(q)) return p;
    const F Z1Z1 = f_sqr(p.Z), Z2Z2 = f_sqr(q.Z);
    const F U1 = f_mul(p.X, Z2Z2), U2 = f_mul(q.X, Z1Z1);
    const F S1 = f_mul(f_mul(p.Y, q.Z), Z2Z2), S2 = f_mul(f_mul(q.Y, p.Z), Z1Z1);
    const F H = f_sub(U2, U1);
    F rr = f_sub(S2, S1);
    if (f_is_zero(H)) {
        if (f_is_zero(rr)) return jac_double(p);
        Jac<F> o = p;
        f_zero(o.Z);
        return o;
    }
    rr = f_add(rr, rr);
    F I = f_add(H, H);
    I = f_sqr(I);
    const F J = f_mul(H, I);
    const F V = f_mul(U1, I);
    Jac<F> r;
    r.X = f_sub(f_sub(f_sqr(rr), J), f_add(V, V));
    F S1J = f_mul(S1, J);
    S1J = f_add(S1J, S1J);
    r.Y = f_sub(f_mul(rr, f_sub(V, r.X)), S1J);
    r.Z = f_mul(f_sub(f_sub(f_sqr(f_add(p.Z, q.Z)), Z1Z1), Z2Z2), H);
    return r;
}
// does the Jacobian point equal the affine point (x, y)?  Infinity equals (0, 0), as the reference's `(0, 0) if None`
template <class F> ZK_HD bool jac_eq_xy(const Jac<F>& p, const F& x, const F& y) {
    if (jac_is_inf(p)) return f_is_zero(x) && f_is_zero(y);
    const F Z2 = f_sqr(p.Z);
    return f_eq(p.X, f_mul(x, Z2)) && f_eq(p.Y, f_mul(y, f_mul(Z2, p.Z)));
}
template <class F> ZK_HD bool aff_eq_xy(const Aff<F>& p, const F& x, const F& y) {
    if (p.inf) return f_is_zero(x) && f_is_zero(y);
    return f_eq(p.x, x) && f_eq(p.y, y);
}

// bit length of the scalar (8 x u32, little-endian)
ZK_HD int scalar_bits(const Fq& n) {
    int nb = 0;
#pragma unroll
    for (int w = 0; w < 8; w++)
        if (n.v[w]) nb = 32 * w + 32 - __builtin_clz(n.v[w]);
    return nb;
}

// py_ecc's multiply(pt, n), exactly:  multiply(pt, n) = multiply(double(pt), n // 2) [+ pt when n is odd], i.e. with
// P_k = double^k(pt) and m = bitlen(n) - 1 the chain is  acc = P_m;  acc = add(acc, P_k) for every set bit k < m, k descending.
// Fast form: P_k = [2^k] pt on the curve y^2 = x^3 + b' through pt (b' = y^2 - x^3: the doubling / addition formulas do not use
// b), in Jacobian coordinates, summed from the low bits up.  The affine chain follows that curve's group law exactly until it
// doubles a point with y = 0 (a 2-torsion point of y^2 = x^3 + b'), where it yields (-2x, 0) instead of infinity; every other
// exceptional step (P + P, P + (-P), None) it handles as the group law does.  Such a step happens iff some P_k with k < m has
// y = 0, which the fast form sees as Y_k = 0 before its doubling: it then reports `*first_zero_y` = k and the caller replays the
// chain (aff_mul_slow).  Points on the curve and on the twist never take it (neither G1 nor E'(Fq2) has a point of order 2).
template <class F> ZK_HD Jac<F> jac_mul_checked(const Aff<F>& pt, const Fq& n, int* first_zero_y) {
    *first_zero_y = -1;
    Jac<F> acc = jac_from_aff(pt);
    f_zero(acc.Z);
    if (pt.inf) return acc;
    const int nb = scalar_bits(n);
    Jac<F> pk = jac_from_aff(pt);
    for (int k = 0; k < nb; k++) {
        if (fq_bit(n, k)) acc = jac_add(acc, pk);
        if (k + 1 < nb) {
            if (f_is_zero(pk.Y)) {
                *first_zero_y = k;
                return acc;
            }
            pk = jac_double(pk);
        }
    }
    return acc;
}
// The replay for a chain whose P_j (j = first_zero_y < m) has y = 0: from there on P_k = ((-2)^(k - j) x_j, 0), so only P_0 .. P_j
// are doublings (each recomputed, the cost is O(j^2) inversions for j at most the 2-adic valuation of the curve's order), the rest
// is closed form, and the additions run in the reference's order.
template <class F> ZK_HD Aff<F> aff_nth_double(const Aff<F>& pt, int k) {
    Aff<F> r = pt;
    for (int i = 0; i < k; i++) r = aff_double(r);
    return r;
}
template <class F> ZK_HD Aff<F> aff_mul_slow(const Aff<F>& pt, const Fq& n, int j) {
    const int m = scalar_bits(n) - 1;
    const Aff<F> pj = aff_nth_double(pt, j);
    Aff<F> tail = pj;  // P_m = ((-2)^(m - j) x_j, 0)
    for (int k = j; k < m; k++) tail.x = f_neg(f_add(tail.x, tail.x));
    Aff<F> acc = tail;
    const Fq inv_neg2 = fq_inv_neg2();
    for (int k = m - 1; k >= 0; k--) {
        Aff<F> pk;
        if (k >= j) {
            tail.x = f_mul_base(tail.x, inv_neg2);
            pk = tail;
        } else {
            pk = aff_nth_double(pt, k);
        }
        if (fq_bit(n, k)) acc = aff_add(acc, pk);
    }
    return acc;
}

// ---- Fq6 / Fq12 ---------------------------------------------------------------------------------------------------------------
ZK_HD Fq6 fq6_make(const Fq2& a, const Fq2& b, const Fq2& c) {
    Fq6 r;
    r.c0 = a;
    r.c1 = b;
    r.c2 = c;
    return r;
}
ZK_HD Fq6 fq6_add(const Fq6& a, const Fq6& b) { return fq6_make(f_add(a.c0, b.c0), f_add(a.c1, b.c1), f_add(a.c2, b.c2)); }
ZK_HD Fq6 fq6_sub(const Fq6& a, const Fq6& b) { return fq6_make(f_sub(a.c0, b.c0), f_sub(a.c1, b.c1), f_sub(a.c2, b.c2)); }
ZK_HD Fq6 fq6_neg(const Fq6& a) { return fq6_make(f_neg(a.c0), f_neg(a.c1), f_neg(a.c2)); }
ZK_HD Fq6 fq6_mul_v(const Fq6& a) { return fq6_make(fq2_mul_xi(a.c2), a.c0, a.c1); }  // times v: v^3 = xi
ZK_NOINLINE Fq6 fq6_mul(const Fq6& a, const Fq6& b) {  // Karatsuba over Fq2 (6 products)
    const Fq2 t0 = f_mul(a.c0, b.c0), t1 = f_mul(a.c1, b.c1), t2 = f_mul(a.c2, b.c2);
    const Fq2 c0 = f_add(t0, fq2_mul_xi(f_sub(f_sub(f_mul(f_add(a.c1, a.c2), f_add(b.c1, b.c2)), t1), t2)));
    const Fq2 c1 = f_add(f_sub(f_sub(f_mul(f_add(a.c0, a.c1), f_add(b.c0, b.c1)), t0), t1), fq2_mul_xi(t2));
    const Fq2 c2 = f_add(f_sub(f_sub(f_mul(f_add(a.c0, a.c2), f_add(b.c0, b.c2)), t0), t2), t1);
    return fq6_make(c0, c1, c2);
}
ZK_HD Fq6 fq6_mul_fq2(const Fq6& a, const Fq2& k) { return fq6_make(f_mul(a.c0, k), f_mul(a.c1, k), f_mul(a.c2, k)); }
// a * (b0 + b1 v): the sparse factor of a line
ZK_NOINLINE Fq6 fq6_mul_01(const Fq6& a, const Fq2& b0, const Fq2& b1) {
    const Fq2 t0 = f_mul(a.c0, b0), t1 = f_mul(a.c1, b1);
    const Fq2 c0 = f_add(t0, fq2_mul_xi(f_mul(a.c2, b1)));
    const Fq2 c1 = f_sub(f_sub(f_mul(f_add(a.c0, a.c1), f_add(b0, b1)), t0), t1);
    const Fq2 c2 = f_add(t1, f_mul(a.c2, b0));
    return fq6_make(c0, c1, c2);
}
ZK_NOINLINE Fq6 fq6_inv(const Fq6& a) {
    const Fq2 t0 = f_sub(f_sqr(a.c0), fq2_mul_xi(f_mul(a.c1, a.c2)));
    const Fq2 t1 = f_sub(fq2_mul_xi(f_sqr(a.c2)), f_mul(a.c0, a.c1));
    const Fq2 t2 = f_sub(f_sqr(a.c1), f_mul(a.c0, a.c2));
    const Fq2 d = f_add(f_mul(a.c0, t0), fq2_mul_xi(f_add(f_mul(a.c2, t1), f_mul(a.c1, t2))));
    const Fq2 di = f_inv(d);
    return fq6_make(f_mul(t0, di), f_mul(t1, di), f_mul(t2, di));
}

ZK_HD Fq12 fq12_one() {
    Fq12 r;
    f_one(r.c0.c0);
    f_zero(r.c0.c1);
    f_zero(r.c0.c2);
    f_zero(r.c1.c0);
    f_zero(r.c1.c1);
    f_zero(r.c1.c2);
    return r;
}
ZK_HD bool fq12_is_one(const Fq12& a) {
    Fq2 one;
    f_one(one);
    return f_eq(a.c0.c0, one) && f_is_zero(a.c0.c1) && f_is_zero(a.c0.c2) && f_is_zero(a.c1.c0) && f_is_zero(a.c1.c1) &&
           f_is_zero(a.c1.c2);
}
ZK_HD Fq12 fq12_make(const Fq6& a, const Fq6& b) {
    Fq12 r;
    r.c0 = a;
    r.c1 = b;
    return r;
}
ZK_NOINLINE Fq12 fq12_mul(const Fq12& a, const Fq12& b) {  // (a0 + a1 w)(b0 + b1 w), w^2 = v
    const Fq6 t0 = fq6_mul(a.c0, b.c0), t1 = fq6_mul(a.c1, b.c1);
    const Fq6 c1 = fq6_sub(fq6_sub(fq6_mul(fq6_add(a.c0, a.c1), fq6_add(b.c0, b.c1)), t0), t1);
    return fq12_make(fq6_add(t0, fq6_mul_v(t1)), c1);
}
ZK_NOINLINE Fq12 fq12_sqr(const Fq12& a) {  // complex squaring: (a0 + a1)(a0 + v a1) - (1 + v) a0 a1, 2 a0 a1 w
    const Fq6 ab = fq6_mul(a.c0, a.c1);
    const Fq6 t = fq6_mul(fq6_add(a.c0, a.c1), fq6_add(a.c0, fq6_mul_v(a.c1)));
    const Fq6 c0 = fq6_sub(fq6_sub(t, ab), fq6_mul_v(ab));
    return fq12_make(c0, fq6_add(ab, ab));
}
ZK_HD Fq12 fq12_conj(const Fq12& a) { return fq12_make(a.c0, fq6_neg(a.c1)); }  // a^(p^6); the inverse in the cyclotomic subgroup
ZK_HD Fq12 fq12_inv(const Fq12& a) {  // (a0 - a1 w) / (a0^2 - v a1^2)
    const Fq6 d = fq6_inv(fq6_sub(fq6_mul(a.c0, a.c0), fq6_mul_v(fq6_mul(a.c1, a.c1))));
    return fq12_make(fq6_mul(a.c0, d), fq6_neg(fq6_mul(a.c1, d)));
}
// f * (c0 + c3 w + c4 v w): the line of a D-type twist (coefficients of w^0, w^1, w^3), 13 Fq2 products instead of 18
ZK_NOINLINE Fq12 fq12_mul_034(const Fq12& f, const Fq2& c0, const Fq2& c3, const Fq2& c4) {
    const Fq6 a = fq6_mul_fq2(f.c0, c0);
    const Fq6 b = fq6_mul_01(f.c1, c3, c4);
    const Fq6 e = fq6_mul_01(fq6_add(f.c0, f.c1), f_add(c0, c3), c4);
    return fq12_make(fq6_add(a, fq6_mul_v(b)), fq6_sub(fq6_sub(e, a), b));
}
// a^p: the coefficient of w^k (w^0, w^2, w^4 in c0; w^1, w^3, w^5 in c1) becomes conj(c) * xi^(k (p - 1) / 6)
ZK_NOINLINE Fq12 fq12_frob(const Fq12& a) {
    const Fq2 g[6] = FQ12_FROB_GAMMA_M;
    Fq12 r;
    r.c0.c0 = fq2_conj(a.c0.c0);
    r.c0.c1 = f_mul(fq2_conj(a.c0.c1), g[2]);
    r.c0.c2 = f_mul(fq2_conj(a.c0.c2), g[4]);
    r.c1.c0 = f_mul(fq2_conj(a.c1.c0), g[1]);
    r.c1.c1 = f_mul(fq2_conj(a.c1.c1), g[3]);
    r.c1.c2 = f_mul(fq2_conj(a.c1.c2), g[5]);
    return r;
}

// ---- optimal ate ---------------------------------------------------------------------------------------------------------
// T in homogeneous projective coordinates (x = X / Z, y = Y / Z) on the twist; the line values are scaled by factors in Fq2,
// which the final exponentiation removes.
struct G2Proj {
    Fq2 X, Y, Z;
};
struct Line {
    Fq2 c0, c3, c4;  // before the evaluation at P: c0 * yP, c3 * xP, c4
};
ZK_HD Fq2 fq2_half(const Fq2& a) {  // a / 2
    const Fq two_inv_neg = fq_inv_neg2();
    return f_neg(f_mul_base(a, two_inv_neg));
}
ZK_NOINLINE Line line_double(G2Proj& t) {
    const Fq2 a = fq2_half(f_mul(t.X, t.Y));
    const Fq2 b = f_sqr(t.Y), c = f_sqr(t.Z);
    const Fq2 e = f_mul(fq2_twist_b(), f_add(f_add(c, c), c));
    const Fq2 ff = f_add(f_add(e, e), e);
    const Fq2 g = fq2_half(f_add(b, ff));
    const Fq2 h = f_sub(f_sqr(f_add(t.Y, t.Z)), f_add(b, c));
    const Fq2 i = f_sub(e, b);
    const Fq2 j = f_sqr(t.X);
    const Fq2 e2 = f_sqr(e);
    t.X = f_mul(a, f_sub(b, ff));
    t.Y = f_sub(f_sqr(g), f_add(f_add(e2, e2), e2));
    t.Z = f_mul(b, h);
    Line l;
    l.c0 = f_neg(h);
    l.c3 = f_add(f_add(j, j), j);
    l.c4 = i;
    return l;
}
ZK_NOINLINE Line line_add(G2Proj& t, const Fq2& qx, const Fq2& qy) {
    const Fq2 theta = f_sub(t.Y, f_mul(qy, t.Z));
    const Fq2 lambda = f_sub(t.X, f_mul(qx, t.Z));
    const Fq2 c = f_sqr(theta), d = f_sqr(lambda);
    const Fq2 e = f_mul(lambda, d), ff = f_mul(t.Z, c), g = f_mul(t.X, d);
    const Fq2 h = f_sub(f_add(e, ff), f_add(g, g));
    t.X = f_mul(lambda, h);
    t.Y = f_sub(f_mul(theta, f_sub(g, h)), f_mul(e, t.Y));
    t.Z = f_mul(t.Z, e);
    Line l;
    l.c0 = lambda;
    l.c3 = f_neg(theta);
    l.c4 = f_sub(f_mul(theta, qx), f_mul(lambda, qy));
    return l;
}
ZK_HD Fq12 line_eval(const Fq12& f, const Line& l, const Fq& px, const Fq& py) {
    return fq12_mul_034(f, f_mul_base(l.c0, py), f_mul_base(l.c3, px), l.c4);
}
// pi(Q) on the twist: (conj(x) xi^((p-1)/3), conj(y) xi^((p-1)/2))
ZK_HD void twist_frob(Fq2& x, Fq2& y) {
    const Fq2 g[6] = FQ12_FROB_GAMMA_M;
    x = f_mul(fq2_conj(x), g[2]);
    y = f_mul(fq2_conj(y), g[3]);
}
// f_{6x+2, Q}(P) * l_{T, pi(Q)}(P) * l_{T', -pi^2(Q)}(P) for P in G1 and Q in G2, both finite (affine, Montgomery form)
ZK_HD Fq12 miller_loop(const Fq& px, const Fq& py, const Fq2& qx, const Fq2& qy) {
    const signed char digits[BN_ATE_LOOP_LEN - 1] = BN_ATE_LOOP_DIGITS;
    G2Proj t;
    t.X = qx;
    t.Y = qy;
    f_one(t.Z);
    const Fq2 nqy = f_neg(qy);
    Fq12 f = fq12_one();
    for (int i = 0; i < BN_ATE_LOOP_LEN - 1; i++) {
        if (i) f = fq12_sqr(f);
        f = line_eval(f, line_double(t), px, py);
        if (digits[i]) f = line_eval(f, line_add(t, qx, digits[i] > 0 ? qy : nqy), px, py);
    }
    Fq2 q1x = qx, q1y = qy;
    twist_frob(q1x, q1y);
    Fq2 q2x = q1x, q2y = q1y;
    twist_frob(q2x, q2y);
    f = line_eval(f, line_add(t, q1x, q1y), px, py);
    f = line_eval(f, line_add(t, q2x, f_neg(q2y)), px, py);
    return f;
}
ZK_HD Fq12 fq12_exp_by_x(const Fq12& a) {  // a^x, x = BN_X_U64 (64-bit square-and-multiply)
    Fq12 r = a;
    for (int bit = 61; bit >= 0; bit--) {  // x has bit 62 as its top bit
        r = fq12_sqr(r);
        if ((BN_X_U64 >> bit) & 1ull) r = fq12_mul(r, a);
    }
    return r;
}
// f^((p^12 - 1) / r) up to a fixed power coprime to r (only "== 1" is observed): the easy part f^((p^6 - 1)(p^2 + 1)), then the
// hard part by the x-chain of Fuentes-Castaneda, Knapp and Rodriguez-Henriquez ("Faster hashing to G2", 2011; the form of
// Aranha et al.'s BN implementations), with conjugation as the inverse in the cyclotomic subgroup.
ZK_HD Fq12 final_exp(const Fq12& f) {
    Fq12 r = fq12_mul(fq12_conj(f), fq12_inv(f));
    r = fq12_mul(fq12_frob(fq12_frob(r)), r);
    const Fq12 y0 = fq12_conj(fq12_exp_by_x(r));  // r^-x
    const Fq12 y1 = fq12_sqr(y0);
    const Fq12 y2 = fq12_sqr(y1);
    Fq12 y3 = fq12_mul(y2, y1);
    const Fq12 y4 = fq12_conj(fq12_exp_by_x(y3));
    const Fq12 y5 = fq12_sqr(y4);
    Fq12 y6 = fq12_conj(fq12_exp_by_x(y5));
    y3 = fq12_conj(y3);
    y6 = fq12_conj(y6);
    const Fq12 y7 = fq12_mul(y6, y4);
    Fq12 y8 = fq12_mul(y7, y3);
    const Fq12 y9 = fq12_mul(y8, y1);
    const Fq12 y10 = fq12_mul(y8, y4);
    const Fq12 y11 = fq12_mul(y10, r);
    const Fq12 y13 = fq12_mul(fq12_frob(y9), y11);
    y8 = fq12_frob(fq12_frob(y8));
    const Fq12 y14 = fq12_mul(y8, y13);
    const Fq12 y15 = fq12_frob(fq12_frob(fq12_frob(fq12_mul(fq12_conj(r), y9))));
    return fq12_mul(y15, y14);
}

}  // namespace bn
