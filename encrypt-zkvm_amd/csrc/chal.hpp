// chal.hpp -- the challenge field of a proof: the base field F (KX = 1, values fe) or its quadratic extension E
// (KX = 2, FieldExtension::Quadratic, values fe2).  Everything after the constraint commitment -- the OOD frame, DEEP,
// FRI -- is written once over Chal<KX>; Chal<1> forwards to the fe_* calls, so the base instantiation of a kernel is
// the base-field kernel.
//
// Layouts over E.  A buffer of M challenge-field values that a later stage reads as base columns (the OOD partial
// sums and frame, the DEEP coefficients and their LDE, FRI layers) is planar: component j at [j M, (j + 1) M), which
// ld / st address as base + j stride.  Kernel-private tables (power tables, g1 / g2, LDS) are arrays of values.
#pragma once
#include "ext2.hpp"

template <int KX>
struct Chal;

template <>
struct Chal<1> {
    typedef fe T;
    typedef acc288 Acc;
    static ZK_HD T zero() { return fe_zero(); }
    static ZK_HD T make(fe2 v) { return v.a; }  // of a lifted value (Coin::draw_ext(1))
    static ZK_HD fe2 wide(T v) { return fe2_lift(v); }
    static ZK_HD fe comp(T v, int) { return v; }
    static ZK_HD T add(T x, T y) { return fe_add(x, y); }
    static ZK_HD T mul(T x, T y) { return fe_mul(x, y); }
    static ZK_HD T mulb(T x, fe s) { return fe_mul(x, s); }
    static ZK_HD T exp(T x, uint64_t e) { return fe_exp(x, e, 0); }
    static ZK_HD T inv(T x) { return fe_inv(x); }
    static ZK_HD T ld(const fe *base, size_t) { return base[0]; }
    static ZK_HD void st(fe *base, size_t, T v) { base[0] = v; }
    // lazy sums of challenge x base products, reduced once
    static ZK_HD Acc acc_zero() { return acc288_zero(); }
    static ZK_HD void madd(Acc &acc, const T &y, fe v) { acc288_madd(acc, y, v); }
    static ZK_HD T reduce(const Acc &acc) { return acc288_reduce(acc); }
};

template <>
struct Chal<2> {
    typedef fe2 T;
    struct Acc {
        acc288 a, b;
    };
    static ZK_HD T zero() { return fe2_zero(); }
    static ZK_HD T make(fe2 v) { return v; }
    static ZK_HD fe2 wide(T v) { return v; }
    static ZK_HD fe comp(T v, int j) { return j ? v.b : v.a; }
    static ZK_HD T add(T x, T y) { return fe2_add(x, y); }
    static ZK_HD T mul(T x, T y) { return fe2_mul(x, y); }
    static ZK_HD T mulb(T x, fe s) { return fe2_mulb(x, s); }
    static ZK_HD T exp(T x, uint64_t e) { return fe2_exp(x, e); }
    static ZK_HD T inv(T x) { return fe2_inv(x); }
    static ZK_HD T ld(const fe *base, size_t stride) { return fe2{base[0], base[stride]}; }
    static ZK_HD void st(fe *base, size_t stride, T v) {
        base[0] = v.a;
        base[stride] = v.b;
    }
    static ZK_HD Acc acc_zero() { return Acc{acc288_zero(), acc288_zero()}; }
    static ZK_HD void madd(Acc &acc, const T &y, fe v) {
        acc288_madd(acc.a, y.a, v);
        acc288_madd(acc.b, y.b, v);
    }
    static ZK_HD T reduce(const Acc &acc) { return fe2{acc288_reduce(acc.a), acc288_reduce(acc.b)}; }
};

// the description of a value type: launchers and helpers that get a point choose their KX by its type
template <class T>
struct ChalOf;
template <>
struct ChalOf<fe> : Chal<1> {
    static constexpr int KX = 1;
};
template <>
struct ChalOf<fe2> : Chal<2> {
    static constexpr int KX = 2;
};

#ifdef __HIPCC__
__device__ __forceinline__ fe wave_sum(fe v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        fe o;
        o.lo = __shfl_xor(v.lo, s, 64);
        o.hi = __shfl_xor(v.hi, s, 64);
        v = fe_add(v, o);
    }
    return v;
}
__device__ __forceinline__ fe2 wave_sum(fe2 v) { return fe2{wave_sum(v.a), wave_sum(v.b)}; }

// sum_e v_e y_e for E base coefficients v and challenge values y: lazy, one reduction per component
template <int E>
__device__ __forceinline__ fe dot_base(const fe *v, const fe *y) {
    acc288 az = acc288_zero();
#pragma unroll
    for (int e = 0; e < E; e++) acc288_madd(az, v[e], y[e]);
    return acc288_reduce(az);
}
template <int E>
__device__ __forceinline__ fe2 dot_base(const fe *v, const fe2 *y) {
    acc288 aa = acc288_zero(), ab = acc288_zero();
#pragma unroll
    for (int e = 0; e < E; e++) {
        const fe2 w = y[e];
        acc288_madd(aa, v[e], w.a);
        acc288_madd(ab, v[e], w.b);
    }
    return fe2{acc288_reduce(aa), acc288_reduce(ab)};
}
#endif
