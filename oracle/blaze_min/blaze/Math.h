// ORACLE — TEST INFRASTRUCTURE ONLY.
//
// A STAND-IN for the third-party linear-algebra library `blaze`.  THIS IS NOT BLAZE and nothing in it comes from blaze: it is this
// project's own code, written from what the reference's KalmanFilter.h asks of the library (the list below) and from this project's
// own description of the evaluation orders (oracle/m17_oracle_dsp.hpp, the comment above Kalman2).  It exists so that the reference's
// KalmanFilter.h, ClockRecovery.h, FreqDevEstimator.h and M17Demodulator.h compile as they lie (oracle/Makefile: -Ioracle/blaze_min
// in front of -I$(REF)/include/m17cxx) and the oracle's restatement of them can be compared with the reference's own text.
//
// What KalmanFilter.h uses, and all that is here:
//   StaticVector<T,N>, StaticMatrix<T,M,N>: brace initialisation, operator() / operator[], assignment from another element type;
//   matrix * matrix, matrix * vector, matrix * scalar;  matrix + matrix, matrix - matrix, scalar - vector, vector += vector;
//   trans(), isnan();  element type of a product or sum = std::common_type of the operands' element types.
// Every sum of products runs k ascending, one rounding per operation in the element type (build with -ffp-contract=off: no FMA).
//
// -DBLAZE_MIN_ORDER=k, k = 0 .. 7, selects how the chained products of KalmanFilter::update are associated: the three bits of the
// oracle's kalman_order() and of m17hip_set_kalman_order().
//   order 0: EAGER.  Every product is evaluated where the source text writes it, left to right, into a temporary of its element
//            type.  `auto S` and `auto K` are plain matrices.
//   bit 0 (x += K*y), bit 1 (P - K*H*P): `auto K = P*trans(H)*s` stays LAZY, as an expression template would: Scaled<Product>.
//            What is then done with K depends on the bit of the statement that uses it; a statement whose bit is clear evaluates K
//            first and goes on as order 0 does.
//   bit 2 (F*P*trans(F)): a chain of three square matrices of one element type is evaluated as A*(B*C), not (A*B)*C.
// Order 3 is "what blaze's documented restructuring rules give" AS THIS PROJECT READS THEM.  That reading is the one thing this file
// cannot vouch for: how blaze itself associates and rounds these products is not pinned by anything here.  What the stand-in pins is
// everything else, namely that the text around the products says what the oracle says it does.
#pragma once

#include <cmath>
#include <cstddef>
#include <initializer_list>
#include <type_traits>

#ifndef BLAZE_MIN_ORDER
#define BLAZE_MIN_ORDER 0
#endif
static_assert(BLAZE_MIN_ORDER >= 0 && BLAZE_MIN_ORDER <= 7, "BLAZE_MIN_ORDER is three bits");

namespace blaze {

template <typename A, typename B>
using Common = std::common_type_t<A, B>;

template <typename T, std::size_t N>
struct StaticVector {
    T v[N] = {};
    StaticVector() = default;
    StaticVector(std::initializer_list<T> l)
    {
        std::size_t i = 0;
        for (T e : l) v[i++] = e;
    }
    template <typename U>
    StaticVector(const StaticVector<U, N>& o) { *this = o; }
    template <typename U>
    StaticVector& operator=(const StaticVector<U, N>& o)   // narrows element by element
    {
        for (std::size_t i = 0; i < N; ++i) v[i] = (T)o.v[i];
        return *this;
    }
    T& operator[](std::size_t i) { return v[i]; }
    const T& operator[](std::size_t i) const { return v[i]; }
    template <typename U>
    StaticVector& operator+=(const StaticVector<U, N>& o)  // x += d: the sum in the common type, narrowed into x
    {
        for (std::size_t i = 0; i < N; ++i) v[i] = (T)((Common<T, U>)v[i] + (Common<T, U>)o.v[i]);
        return *this;
    }
};

template <typename T, std::size_t M, std::size_t N>
struct StaticMatrix {
    T a[M][N] = {};
    StaticMatrix() = default;
    StaticMatrix(std::initializer_list<std::initializer_list<T>> rows)
    {
        std::size_t i = 0;
        for (const auto& r : rows) {
            std::size_t j = 0;
            for (T e : r) a[i][j++] = e;
            ++i;
        }
    }
    template <typename U>
    StaticMatrix(const StaticMatrix<U, M, N>& o) { *this = o; }
    template <typename U>
    StaticMatrix& operator=(const StaticMatrix<U, M, N>& o)  // narrows element by element
    {
        for (std::size_t i = 0; i < M; ++i)
            for (std::size_t j = 0; j < N; ++j) a[i][j] = (T)o.a[i][j];
        return *this;
    }
    T& operator()(std::size_t i, std::size_t j) { return a[i][j]; }
    const T& operator()(std::size_t i, std::size_t j) const { return a[i][j]; }
};

// ---- eager kernels --------------------------------------------------------------------------------------------------------------
template <typename T, typename U, std::size_t M, std::size_t K, std::size_t N>
inline StaticMatrix<Common<T, U>, M, N> mul(const StaticMatrix<T, M, K>& l, const StaticMatrix<U, K, N>& r)
{
    using C = Common<T, U>;
    StaticMatrix<C, M, N> o;
    for (std::size_t i = 0; i < M; ++i)
        for (std::size_t j = 0; j < N; ++j) {
            C s = (C)l.a[i][0] * (C)r.a[0][j];
            for (std::size_t k = 1; k < K; ++k) s = s + (C)l.a[i][k] * (C)r.a[k][j];
            o.a[i][j] = s;
        }
    return o;
}

template <typename T, typename U, std::size_t M, std::size_t N>
inline StaticVector<Common<T, U>, M> operator*(const StaticMatrix<T, M, N>& l, const StaticVector<U, N>& r)
{
    using C = Common<T, U>;
    StaticVector<C, M> o;
    for (std::size_t i = 0; i < M; ++i) {
        C s = (C)l.a[i][0] * (C)r.v[0];
        for (std::size_t k = 1; k < N; ++k) s = s + (C)l.a[i][k] * (C)r.v[k];
        o.v[i] = s;
    }
    return o;
}

template <typename T, typename S, std::size_t M, std::size_t N, typename = std::enable_if_t<std::is_arithmetic<S>::value>>
inline StaticMatrix<Common<T, S>, M, N> scale(const StaticMatrix<T, M, N>& l, S s)
{
    using C = Common<T, S>;
    StaticMatrix<C, M, N> o;
    for (std::size_t i = 0; i < M; ++i)
        for (std::size_t j = 0; j < N; ++j) o.a[i][j] = (C)l.a[i][j] * (C)s;
    return o;
}

template <typename T, typename U, std::size_t M, std::size_t N>
inline StaticMatrix<Common<T, U>, M, N> operator+(const StaticMatrix<T, M, N>& l, const StaticMatrix<U, M, N>& r)
{
    using C = Common<T, U>;
    StaticMatrix<C, M, N> o;
    for (std::size_t i = 0; i < M; ++i)
        for (std::size_t j = 0; j < N; ++j) o.a[i][j] = (C)l.a[i][j] + (C)r.a[i][j];
    return o;
}

template <typename T, typename U, std::size_t M, std::size_t N>
inline StaticMatrix<Common<T, U>, M, N> operator-(const StaticMatrix<T, M, N>& l, const StaticMatrix<U, M, N>& r)
{
    using C = Common<T, U>;
    StaticMatrix<C, M, N> o;
    for (std::size_t i = 0; i < M; ++i)
        for (std::size_t j = 0; j < N; ++j) o.a[i][j] = (C)l.a[i][j] - (C)r.a[i][j];
    return o;
}

template <typename S, typename T, std::size_t N, typename = std::enable_if_t<std::is_arithmetic<S>::value>>
inline StaticVector<Common<S, T>, N> operator-(S s, const StaticVector<T, N>& r)   // scalar - vector, element by element
{
    using C = Common<S, T>;
    StaticVector<C, N> o;
    for (std::size_t i = 0; i < N; ++i) o.v[i] = (C)s - (C)r.v[i];
    return o;
}

template <typename T, std::size_t M, std::size_t N>
inline StaticMatrix<T, N, M> trans(const StaticMatrix<T, M, N>& m)
{
    StaticMatrix<T, N, M> o;
    for (std::size_t i = 0; i < M; ++i)
        for (std::size_t j = 0; j < N; ++j) o.a[j][i] = m.a[i][j];
    return o;
}

template <typename T, std::size_t N>
inline bool isnan(const StaticVector<T, N>& x)   // any element
{
    for (std::size_t i = 0; i < N; ++i)
        if (std::isnan(x.v[i])) return true;
    return false;
}

// ---- expressions ----------------------------------------------------------------------------------------------------------------
// Product: A*B not yet evaluated (operands held by value: they are 2 x 2 at most, and the statement may assign to one of them).
template <typename T, typename U, std::size_t M, std::size_t K, std::size_t N>
struct Product {
    StaticMatrix<T, M, K> l;
    StaticMatrix<U, K, N> r;
    StaticMatrix<Common<T, U>, M, N> eval() const { return mul(l, r); }
};

// ScaledProduct: (A*B)*s with A*B not yet evaluated — what `auto K` holds when bit 0 or bit 1 is set.
template <typename T, typename U, typename S, std::size_t M, std::size_t K, std::size_t N>
struct ScaledProduct {
    Product<T, U, M, K, N> p;
    S s;
    StaticMatrix<Common<Common<T, U>, S>, M, N> eval() const { return scale(p.eval(), s); }   // the eager K
};

// ScaledMatrix: G*s with G evaluated — the two steps of bit 1 pass the scalar along in it.
template <typename T, typename S, std::size_t M, std::size_t N>
struct ScaledMatrix {
    StaticMatrix<T, M, N> g;
    S s;
    StaticMatrix<Common<T, S>, M, N> eval() const { return scale(g, s); }
};

// A * B
template <typename T, typename U, std::size_t M, std::size_t K, std::size_t N>
inline Product<T, U, M, K, N> operator*(const StaticMatrix<T, M, K>& l, const StaticMatrix<U, K, N>& r)
{
    return {l, r};
}

// (A*B) * C.  Stands for: a chain of three matrices.  Bit 2 set and all three square of one element type (F*P*trans(F), the only
// such chain in KalmanFilter.h): A*(B*C), the right product into a temporary first.  Otherwise as C++ parses it: (A*B) into a
// temporary of its element type, then times C.  H*P*trans(H) and K*H*P are not of that shape and keep the parse order under every order.
template <typename T, typename U, typename V, std::size_t M, std::size_t K, std::size_t L, std::size_t N>
inline auto operator*(const Product<T, U, M, K, L>& p, const StaticMatrix<V, L, N>& c)
{
    if constexpr ((BLAZE_MIN_ORDER & 4) != 0 && std::is_same<T, U>::value && std::is_same<U, V>::value && M == K && K == L && L == N)
        return Product<T, Common<U, V>, M, K, N>{p.l, mul(p.r, c)};
    else
        return Product<Common<T, U>, V, M, L, N>{p.eval(), c};
}

// (A*B) + C, C - (A*B): evaluate the product, then element by element.
template <typename T, typename U, typename V, std::size_t M, std::size_t K, std::size_t N>
inline auto operator+(const Product<T, U, M, K, N>& p, const StaticMatrix<V, M, N>& c)
{
    return p.eval() + c;
}
template <typename T, typename U, typename V, std::size_t M, std::size_t K, std::size_t N>
inline auto operator-(const StaticMatrix<V, M, N>& c, const Product<T, U, M, K, N>& p)
{
    return c - p.eval();
}

// (A*B) * s.  Order 0: evaluate A*B, scale it: a matrix of the common type.  Otherwise it stays an expression.
template <typename T, typename U, typename S, std::size_t M, std::size_t K, std::size_t N, typename = std::enable_if_t<std::is_arithmetic<S>::value>>
inline auto operator*(const Product<T, U, M, K, N>& p, S s)
{
    if constexpr ((BLAZE_MIN_ORDER & 3) == 0)
        return scale(p.eval(), s);
    else
        return ScaledProduct<T, U, S, M, K, N>{p, s};
}

// ((A*B)*s) * v.  Bit 0 stands for two restructurings in a row: (X*s)*v -> (X*v)*s, then (A*B)*v -> A*(B*v): both products in the
// matrices' element type, the scalar last.  Bit 0 clear: K evaluated, then K*v.
template <typename T, typename U, typename S, typename V, std::size_t M, std::size_t K, std::size_t N>
inline auto operator*(const ScaledProduct<T, U, S, M, K, N>& k, const StaticVector<V, N>& v)
{
    if constexpr ((BLAZE_MIN_ORDER & 1) != 0) {
        using E = Common<Common<T, U>, V>;
        using C = Common<E, S>;
        const StaticVector<E, M> t = k.p.l * (k.p.r * v);
        StaticVector<C, M> o;
        for (std::size_t i = 0; i < M; ++i) o.v[i] = (C)t.v[i] * (C)k.s;
        return o;
    } else
        return k.eval() * v;
}

// ((A*B)*s) * C.  Bit 1 stands for (X*s)*C -> (X*C)*s with X = A*B evaluated on the way: G = (A*B)*C in the matrices' element
// type, the scalar kept aside.  Bit 1 clear: K evaluated, then the product K*C as above.
template <typename T, typename U, typename S, typename V, std::size_t M, std::size_t K, std::size_t L, std::size_t N>
inline auto operator*(const ScaledProduct<T, U, S, M, K, L>& k, const StaticMatrix<V, L, N>& c)
{
    if constexpr ((BLAZE_MIN_ORDER & 2) != 0)
        return ScaledMatrix<Common<Common<T, U>, V>, S, M, N>{mul(k.p.eval(), c), k.s};
    else
        return k.eval() * c;
}

// (G*s) * C -> (G*C)*s: the second step of bit 1 (only reached with bit 1 set).
template <typename T, typename S, typename V, std::size_t M, std::size_t K, std::size_t N>
inline ScaledMatrix<Common<T, V>, S, M, N> operator*(const ScaledMatrix<T, S, M, K>& g, const StaticMatrix<V, K, N>& c)
{
    return {mul(g.g, c), g.s};
}

// C - G*s: the scaling and the difference element by element in the common type.
template <typename T, typename S, typename V, std::size_t M, std::size_t N>
inline auto operator-(const StaticMatrix<V, M, N>& c, const ScaledMatrix<T, S, M, N>& g)
{
    return c - g.eval();
}

}  // namespace blaze
