// The f32 transcendentals of geo_math.h (asinf_, acosf_, acos_pi_, sincosf_,
// sincos_sky_, atanf_, atan2f_, atan2_turns_), swept on the GPU.  For the
// function named on the command line, over its input set:
//  (a) bits: the device's results against the host build of the same header.
//      The kernel sums, per chunk of 2^16 consecutive inputs, a 64-bit mix of
//      (input index, result bits), a bijection of the result bits for a fixed
//      input, so the wrapping sum changes when one result bit of one input
//      does.  Any NaN result is one token; every other result counts by its
//      bits (the sign of zero too).  The host recomputes the digests on at
//      most 16 threads; a differing chunk is re-run input by input against a
//      device copy of its results.  Prints "mismatches N".
//  (b) accuracy: the device's results against the device's f64 library
//      function on the widened input, the worst error per binade of the input
//      in the function's own unit, over the function's stated domain, and the
//      range properties over every input.  Prints the table, "worst",
//      "range_violations N".
// Input sets.  One argument: every f32 bit pattern; the index is the pattern.
// atan2f_ and atan2_turns_ (y, x), by index n:
//   n < 4 * 2^32              (t, +1), (t, -1), (+1, t), (-1, t): n >> 32
//                             names the form, t is the low word's pattern;
//   then 2^26 entries         (t s, s) and (s, t s) for s = 2^-60, 2^60 on
//                             every 256th t with 2^-30 <= |t| <= 2^30 (other
//                             t are left out); the low 2 bits name the form;
//   then 2^24 entries         (+-0, +-0), then pairs from a counter hash with
//                             independent signs and exponents in [-60, 60].
// The accuracy bars of the two-argument forms apply where max(|x|, |y|) is in
// [2^-60, 2^61).
//
// Modes:
//   FUNC [--part K N] [--oracle LIB] [--mutate INDEX] [--no-device]
//         the GPU sweep, (a) and (b), on the K-th of N equal parts of the
//         chunks.  --oracle: the host pass also compares the host header with
//         the oracle's exported mirror in LIB (liboracle.so), bit for bit on
//         every input, and prints "oracle mismatches N"; with --no-device
//         that is all it does.  --mutate flips the low result bit of that one
//         input on the device side (here, not in geo_math.h): the sweep must
//         then report it and exit with status 1.
//   FUNC --host [--oracle LIB] [--threads T]   no GPU (the only mode of a
//         host-only build, g++ -x c++): a subset of the inputs (every 64th
//         pattern and +-4096 patterns around each edge) against the host's
//         libm in f64, the range properties, and the oracle's mirror.
// Exit status: 0 iff no mismatch (accuracy is asserted by the caller from the
// printed figures); 2 on a usage or runtime error.
#if defined(__HIP__)
#include <hip/hip_runtime.h>
#endif
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../schwarzschild_raytracer_wgpu_amd/csrc/geo_math.h"

#if defined(__HIP__)
#define TX_HD __host__ __device__ inline
#else
#define TX_HD inline
#endif

enum Fn { kAsin, kAcos, kAcosPi, kSincos, kSincosSky, kAtan, kAtan2, kAtan2Turns, kFnCount };
static const char* const kFnName[kFnCount] = {"asinf_",      "acosf_", "acos_pi_", "sincosf_",
                                              "sincos_sky_", "atanf_", "atan2f_",  "atan2_turns_"};

constexpr uint64_t kChunk = 1ull << 16;
constexpr uint64_t kNoMutate = ~0ull;
constexpr uint64_t kForms = 4ull << 32;         // the two-argument sets: the four (t, +-1) forms,
constexpr uint64_t kScaled = 1ull << 26;        // the scaled pairs,
constexpr uint64_t kRandom = 1ull << 24;        // the zeros and the hashed pairs
constexpr uint32_t kNanToken = 0x7fc00000u;

TX_HD bool two_args(int f) { return f == kAtan2 || f == kAtan2Turns; }
TX_HD uint64_t total_inputs(int f) { return two_args(f) ? kForms + kScaled + kRandom : 1ull << 32; }

TX_HD uint32_t f2u(float x) { return __builtin_bit_cast(uint32_t, x); }
TX_HD float u2f(uint32_t b) { return __builtin_bit_cast(float, b); }
TX_HD uint64_t mix64(uint64_t v) {  // splitmix64's finaliser: a bijection
    v ^= v >> 30;
    v *= 0xbf58476d1ce4e5b9ull;
    v ^= v >> 27;
    v *= 0x94d049bb133111ebull;
    return v ^ (v >> 31);
}

// Input n of function f.  False: n names no input (a t outside the scaled set).
TX_HD bool gen(int f, uint64_t n, float* a, float* b) {
    *b = 0.0f;
    if (!two_args(f)) {
        *a = u2f((uint32_t)n);
        return true;
    }
    if (n < kForms) {
        const float t = u2f((uint32_t)n);
        switch ((int)(n >> 32)) {
            case 0: *a = t, *b = 1.0f; break;
            case 1: *a = t, *b = -1.0f; break;
            case 2: *a = 1.0f, *b = t; break;
            default: *a = -1.0f, *b = t; break;
        }
        return true;
    }
    n -= kForms;
    if (n < kScaled) {
        const float t = u2f((uint32_t)(n >> 2) << 8);
        const float at = __builtin_fabsf(t);
        if (!(at >= 0x1p-30f && at <= 0x1p30f)) return false;
        const float s = (n & 1) ? 0x1p60f : 0x1p-60f;
        if (n & 2) *a = s, *b = t * s;
        else *a = t * s, *b = s;
        return true;
    }
    n -= kScaled;
    if (n < 4) {
        *a = (n & 1) ? -0.0f : 0.0f;
        *b = (n & 2) ? -0.0f : 0.0f;
        return true;
    }
    const uint64_t h0 = mix64(n + 0x9e3779b97f4a7c15ull), h1 = mix64(h0 + 0x9e3779b97f4a7c15ull);
    const uint32_t ey = (uint32_t)((h0 >> 32) % 121u) + 67u, ex = (uint32_t)((h1 >> 32) % 121u) + 67u;  // 127 - 60 ..
    *a = u2f(((uint32_t)h0 & 0x807fffffu) | (ey << 23));
    *b = u2f(((uint32_t)h1 & 0x807fffffu) | (ex << 23));
    return true;
}

// The function's result bits (o[1] = 0 for a function of one result).
TX_HD void eval(int f, float a, float b, uint32_t o[2]) {
    float r0 = 0.0f, r1 = 0.0f;
    switch (f) {
        case kAsin: r0 = geo::asinf_(a); break;
        case kAcos: r0 = geo::acosf_(a); break;
        case kAcosPi: r0 = geo::acos_pi_(a); break;
        case kSincos: geo::sincosf_(a, &r0, &r1); break;
        case kSincosSky: geo::sincos_sky_(a, &r0, &r1); break;
        case kAtan: r0 = geo::atanf_(a); break;
        case kAtan2: r0 = geo::atan2f_(a, b); break;
        default: r0 = geo::atan2_turns_(a, b); break;
    }
    o[0] = f2u(r0);
    o[1] = f2u(r1);
}

TX_HD uint64_t digest_term(uint64_t n, const uint32_t o[2]) {
    const uint32_t t0 = (o[0] & 0x7fffffffu) > 0x7f800000u ? kNanToken : o[0];
    const uint32_t t1 = (o[1] & 0x7fffffffu) > 0x7f800000u ? kNanToken : o[1];
    return mix64((((uint64_t)t0 << 32) | t1) ^ (n * 0x9e3779b97f4a7c15ull));
}

// One unit in the last place of |ref| rounded to f32 (numpy's spacing).
TX_HD double ulp_of(double ref) {
    const float f = (float)fabs(ref);
    return (double)u2f(f2u(f) + 1u) - (double)f;
}

struct Acc {
    uint64_t digest;
    uint64_t range_bad;   // inputs that break a range property
    uint64_t n_acc;       // inputs measured in (b)
    double worst[2];      // [0]: over the stated domain; [1]: sincos_sky_ on [-7, fl(pi/2) + 2^-20]
    uint64_t at[2];       // the input index of each
};

TX_HD void acc_init(Acc& k) {
    k.digest = k.range_bad = k.n_acc = 0;
    k.worst[0] = k.worst[1] = -1.0;
    k.at[0] = k.at[1] = 0;
}
TX_HD void acc_worst(Acc& k, int i, double e, uint64_t n) {
    if (!(e == e)) e = INFINITY;
    if (e > k.worst[i] || (e == k.worst[i] && n < k.at[i])) k.worst[i] = e, k.at[i] = n;
}
TX_HD void acc_merge(Acc& k, const Acc& o) {
    k.digest += o.digest;
    k.range_bad += o.range_bad;
    k.n_acc += o.n_acc;
    for (int i = 0; i < 2; ++i)
        if (o.worst[i] >= 0.0) acc_worst(k, i, o.worst[i], o.at[i]);
}

// The accuracy of result o for input (a, b) against the f64 library (the
// device's in a kernel, the host's elsewhere), and the range properties.
TX_HD void measure(int f, uint64_t n, float a, float b, const uint32_t o[2], Acc& k) {
    const float r0 = u2f(o[0]), r1 = u2f(o[1]);
    const double x = (double)a, got = (double)r0;
    const float aa = __builtin_fabsf(a);
    const bool a_nan = a != a, b_nan = b != b;
    switch (f) {
        case kAsin: {
            if (a_nan || aa > 1.0f) {  // +-fl(pi/2) by the sign bit
                if (o[0] != ((f2u(a) & 0x80000000u) | f2u(geo::kPi2))) ++k.range_bad;
                return;
            }
            const double ref = asin(x);
            const double d = fabs(got - ref) - 1e-12;
            ++k.n_acc;
            acc_worst(k, 0, (d > 0.0 ? d : (d == d ? 0.0 : d)) / ulp_of(ref), n);
            return;
        }
        case kAcos: {
            if (a_nan || aa > 1.0f) return;
            const double ref = acos(x);
            ++k.n_acc;
            acc_worst(k, 0, fabs(got - ref) / ulp_of(ref), n);
            return;
        }
        case kAcosPi: {
            if (!(r0 >= 0.0f && r0 <= 1.0f)) ++k.range_bad;
            if (a_nan || aa > 1.0f) return;
            ++k.n_acc;
            acc_worst(k, 0, fabs(got - acos(x) / 3.14159265358979323846), n);
            return;
        }
        case kSincos:
        case kSincosSky: {
            if (a_nan || !(aa < (f == kSincos ? 1e4f : 0x1p21f))) return;
            const double es = fabs(got - sin(x)), ec = fabs((double)r1 - cos(x));
            const double e = (es == es && ec == ec) ? (es > ec ? es : ec) : NAN;
            ++k.n_acc;
            acc_worst(k, 0, e, n);
            if (f == kSincosSky && a >= -7.0f && a <= geo::kPi2 + 0x1p-20f) acc_worst(k, 1, e, n);
            return;
        }
        default: break;
    }
    // atanf_ (x = 1), atan2f_, atan2_turns_
    const float y = a, xx = f == kAtan ? 1.0f : b;
    if (a_nan || b_nan) return;
    if (f == kAtan2Turns) {
        bool bad = !(r0 >= 0.0f && r0 <= 1.0f) || o[0] == 0x80000000u;
        if (y == 0.0f && f2u(xx) == 0u && o[0] != 0u) bad = true;  // atan2(+-0, 0) = 0
        if (bad) ++k.range_bad;
    }
    const float m = __builtin_fmaxf(__builtin_fabsf(y), __builtin_fabsf(xx));
    if (!(m >= 0x1p-60f && m < 0x1p61f)) return;
    const double ref = atan2((double)y, (double)xx);
    ++k.n_acc;
    if (f == kAtan2Turns) {
        double t = ref / 6.28318530717958647692;
        if (t < 0.0) t += 1.0;
        const double d = fabs(got - t);
        acc_worst(k, 0, d < 1.0 - d ? d : 1.0 - d, n);
    } else {
        const double d = fabs(got - ref) - 1e-9;
        acc_worst(k, 0, (d > 0.0 ? d : (d == d ? 0.0 : d)) / ulp_of(ref), n);
    }
}

// Input n: its digest term, and with `accuracy` its measurements, into k.
TX_HD void visit(int f, uint64_t n, uint64_t mutate, bool accuracy, Acc& k) {
    float a, b;
    if (!gen(f, n, &a, &b)) return;
    GEO_OPAQUE(a);
    GEO_OPAQUE(b);
    uint32_t o[2];
    eval(f, a, b, o);
    if (n == mutate) o[0] ^= 1u;
    k.digest += digest_term(n, o);
    if (accuracy) measure(f, n, a, b, o, k);
}

#if defined(__HIP__)
// One workgroup per chunk (grid-stride over the chunks c0 .. c1), 256 inputs a lane.
template <int F>
__global__ __launch_bounds__(256) void sweep(uint64_t c0, uint64_t c1, uint64_t mutate, Acc* out) {
    __shared__ Acc part[256];
    for (uint64_t c = c0 + blockIdx.x; c < c1; c += gridDim.x) {
        Acc k;
        acc_init(k);
        for (uint32_t i = threadIdx.x; i < kChunk; i += 256u) visit(F, c * kChunk + i, mutate, true, k);
        part[threadIdx.x] = k;
        __syncthreads();
        for (uint32_t s = 128u; s > 0u; s >>= 1) {
            if (threadIdx.x < s) acc_merge(part[threadIdx.x], part[threadIdx.x + s]);
            __syncthreads();
        }
        if (threadIdx.x == 0) out[c - c0] = part[0];
        __syncthreads();
    }
}

// The result bits of chunk c, input by input (for a chunk whose digest differs).
template <int F>
__global__ __launch_bounds__(256) void dump(uint64_t c, uint64_t mutate, uint32_t* out) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= kChunk) return;
    const uint64_t n = c * kChunk + i;
    float a, b;
    uint32_t o[2] = {0u, 0u};
    if (gen(F, n, &a, &b)) {
        GEO_OPAQUE(a);
        GEO_OPAQUE(b);
        eval(F, a, b, o);
        if (n == mutate) o[0] ^= 1u;
    }
    out[2 * i] = o[0];
    out[2 * i + 1] = o[1];
}

template <int F>
static void launch_sweep(uint64_t c0, uint64_t c1, uint64_t mutate, Acc* out) {
    const uint64_t nc = c1 - c0;
    hipLaunchKernelGGL(sweep<F>, dim3((unsigned)std::min<uint64_t>(nc, 256u * 32u)), dim3(256), 0, 0, c0, c1, mutate,
                       out);
}
template <int F>
static void launch_dump(uint64_t c, uint64_t mutate, uint32_t* out) {
    hipLaunchKernelGGL(dump<F>, dim3((unsigned)(kChunk / 256u)), dim3(256), 0, 0, c, mutate, out);
}
typedef void (*SweepFn)(uint64_t, uint64_t, uint64_t, Acc*);
typedef void (*DumpFn)(uint64_t, uint64_t, uint32_t*);
static const SweepFn kSweep[kFnCount] = {launch_sweep<kAsin>,      launch_sweep<kAcos>, launch_sweep<kAcosPi>,
                                         launch_sweep<kSincos>,    launch_sweep<kSincosSky>,
                                         launch_sweep<kAtan>,      launch_sweep<kAtan2>,
                                         launch_sweep<kAtan2Turns>};
static const DumpFn kDump[kFnCount] = {launch_dump<kAsin>,   launch_dump<kAcos>, launch_dump<kAcosPi>,
                                       launch_dump<kSincos>, launch_dump<kSincosSky>,
                                       launch_dump<kAtan>,   launch_dump<kAtan2>,
                                       launch_dump<kAtan2Turns>};
#endif

// ---- the host side ----

static void describe(int f, uint64_t n, char* buf, size_t len) {
    float a = 0.0f, b = 0.0f;
    gen(f, n, &a, &b);
    if (two_args(f))
        snprintf(buf, len, "index 0x%llx (y = 0x%08x %.9g, x = 0x%08x %.9g)", (unsigned long long)n, f2u(a), a, f2u(b),
                 b);
    else
        snprintf(buf, len, "index 0x%llx (x = 0x%08x %.9g)", (unsigned long long)n, f2u(a), a);
}

// Runs fn(t) on T threads.
template <class Fn_>
static void on_threads(unsigned T, Fn_ fn) {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < T; ++t) th.emplace_back(fn, t);
    for (auto& x : th) x.join();
}

// The row of the table an input falls in: the exponent field of the input
// (of t in the two-argument forms), 256 for the scaled pairs' chunk, 257 for
// the zeros and hashed pairs.
static int row_of(int f, uint64_t n) {
    if (two_args(f) && n >= kForms) return n < kForms + kScaled ? 256 : 257;
    return (int)(((uint32_t)n >> 23) & 255u);
}

struct Table {
    Acc row[258];
    Acc all;
    Table() {
        for (auto& r : row) acc_init(r);
        acc_init(all);
    }
    void add(int f, uint64_t first_input, const Acc& k) {
        acc_merge(row[row_of(f, first_input)], k);
        acc_merge(all, k);
    }
    void merge(const Table& o) {
        for (int i = 0; i < 258; ++i) acc_merge(row[i], o.row[i]);
        acc_merge(all, o.all);
    }
};

static const char* unit_of(int f) {
    switch (f) {
        case kAsin: return "ulp(ref) after 1e-12";
        case kAcos: return "ulp(ref)";
        case kAtan:
        case kAtan2: return "ulp(ref) after 1e-9";
        case kAtan2Turns: return "turns, circular";
        default: return "absolute";
    }
}

static void print_table(int f, const Table& t, const char* ref_name) {
    char buf[160];
    printf("function %s reference %s unit %s\n", kFnName[f], ref_name, unit_of(f));
    for (int i = 0; i < 258; ++i) {
        const Acc& r = t.row[i];
        if (r.n_acc == 0) continue;
        describe(f, r.at[0], buf, sizeof buf);
        if (i < 256)
            printf("binade %d count %llu worst %.6e at %s\n", i - 127, (unsigned long long)r.n_acc, r.worst[0], buf);
        else
            printf("set %s count %llu worst %.6e at %s\n", i == 256 ? "scaled" : "hashed", (unsigned long long)r.n_acc,
                   r.worst[0], buf);
    }
    if (t.all.n_acc) {
        describe(f, t.all.at[0], buf, sizeof buf);
        printf("worst %.6e at %s\n", t.all.worst[0], buf);
    } else {
        printf("worst 0 at none\n");
    }
    if (f == kSincosSky && t.all.worst[1] >= 0.0) {
        describe(f, t.all.at[1], buf, sizeof buf);
        printf("worst_sampled_range %.6e at %s\n", t.all.worst[1], buf);
    }
    printf("measured %llu\n", (unsigned long long)t.all.n_acc);
    printf("range_violations %llu\n", (unsigned long long)t.all.range_bad);
}

// The oracle's mirror of function f as eval() (nullptr: it exports none).
struct Mirror {
    float (*f1)(float) = nullptr;
    float (*f2)(float, float) = nullptr;
    void (*sc)(float, float*, float*) = nullptr;
    int f = 0;
    bool load(const char* lib, int fn) {
        f = fn;
        void* h = dlopen(lib, RTLD_NOW | RTLD_LOCAL);
        if (!h) {
            fprintf(stderr, "dlopen %s: %s\n", lib, dlerror());
            return false;
        }
        const char* name = nullptr;
        switch (fn) {
            case kAsin: name = "geo_oracle_asinf"; break;
            case kAcosPi: name = "geo_oracle_acos_pi"; break;
            case kSincos: name = "geo_oracle_sincosf"; break;
            case kSincosSky: name = "geo_oracle_sincos_sky"; break;
            case kAtan:
            case kAtan2: name = "geo_oracle_atan2f"; break;
            case kAtan2Turns: name = "geo_oracle_atan2_turns"; break;
            default: return false;  // acosf_ has no exported mirror
        }
        void* p = dlsym(h, name);
        if (!p) {
            fprintf(stderr, "dlsym %s failed\n", name);
            return false;
        }
        if (fn == kSincos || fn == kSincosSky) sc = (void (*)(float, float*, float*))p;
        else if (fn == kAsin || fn == kAcosPi) f1 = (float (*)(float))p;
        else f2 = (float (*)(float, float))p;
        return true;
    }
    void eval(float a, float b, uint32_t o[2]) const {
        float r0 = 0.0f, r1 = 0.0f;
        if (sc) sc(a, &r0, &r1);
        else if (f1) r0 = f1(a);
        else r0 = f2(a, f == kAtan ? 1.0f : b);
        o[0] = f2u(r0);
        o[1] = f2u(r1);
    }
};

// Where the mirror restates the header.  sincosf_ takes j = rint(x 2/pi) and
// its quadrant from the 1.5 * 2^23 shifter, the mirror from rintf and an int
// cast: the same for |x 2/pi| < 2^22, |x| < 6.5e6 (flr_exhaustive.hip's
// domain; the function is specified for |x| < 1e4).  Past it the shifter
// holds no integer and the cast of j >= 2^31 is undefined.
static bool mirrored(int f, float a) { return f != kSincos || a != a || __builtin_fabsf(a) < 6.5e6f; }

struct Diff {
    uint64_t n;
    uint32_t want[2], got[2];
};
static bool same_token(const uint32_t p[2], const uint32_t q[2]) {
    for (int i = 0; i < 2; ++i) {
        const bool pn = (p[i] & 0x7fffffffu) > 0x7f800000u, qn = (q[i] & 0x7fffffffu) > 0x7f800000u;
        if (pn != qn || (!pn && p[i] != q[i])) return false;
    }
    return true;
}
static void print_diffs(int f, const std::vector<Diff>& d, const char* want, const char* got) {
    char buf[160];
    for (size_t i = 0; i < d.size() && i < 8; ++i) {
        describe(f, d[i].n, buf, sizeof buf);
        printf("  %s: %s 0x%08x 0x%08x, %s 0x%08x 0x%08x\n", buf, want, d[i].want[0], d[i].want[1], got, d[i].got[0],
               d[i].got[1]);
    }
}

// ---- the host subset (--host) ----

static void push_edge(std::vector<uint32_t>& v, float x) {
    v.push_back(f2u(x));
    v.push_back(f2u(-x));
}
// The bit patterns around which +-4096 neighbours are visited.
static std::vector<uint32_t> edges() {
    std::vector<uint32_t> v;
    push_edge(v, 0.0f);
    push_edge(v, u2f(1u));           // denormal min
    push_edge(v, u2f(0x007fffffu));  // denormal max
    push_edge(v, 0.5f);
    push_edge(v, 1.0f);
    for (int k = 1; k <= 8; ++k) push_edge(v, geo::kPi2 * (float)k);
    push_edge(v, 0.4142135623730950f);  // tan(pi/8), tan(3 pi/8): atan2's `mid` and `big`
    push_edge(v, 2.414213562373095f);
    push_edge(v, 1e4f);
    push_edge(v, 0x1p21f);
    push_edge(v, 0x1p-60f);
    push_edge(v, 0x1p60f);
    push_edge(v, 0.501707613f);  // the worst inputs of the exhaustive host sweep
    push_edge(v, 7.85337734f);
    push_edge(v, 0x1p-126f);
    v.push_back(0x7f800000u);  // +-inf and the signaling NaNs next to them (0x7f800001..: a host fminf
    v.push_back(0xff800000u);  // answered them with NaN where the device clamps |x| to 1; geo_math.h min_nan_b_)
    v.push_back(0x7fc00000u);  // the quiet NaNs and the last signaling ones
    v.push_back(0xffc00000u);
    return v;
}

// Calls fn(n) for every input index of the subset that thread t of T owns.
template <class Fn_>
static void subset(int f, unsigned t, unsigned T, Fn_ fn) {
    const uint64_t forms = two_args(f) ? 4 : 1;
    const std::vector<uint32_t> e = edges();
    for (uint64_t s = 0; s < forms; ++s) {
        for (uint64_t p = t; p < (1ull << 26); p += T) fn((s << 32) | (p << 6));
        for (size_t i = t; i < e.size(); i += T)
            for (int64_t d = -4096; d <= 4096; ++d) {
                const uint32_t p = (uint32_t)((int64_t)e[i] + d);
                if ((p & 63u) == 0u) continue;  // visited above
                fn((s << 32) | p);
            }
    }
    if (two_args(f))
        for (uint64_t n = kForms + t; n < kForms + kScaled + kRandom; n += T) fn(n);
}

static int run_host(int f, const char* lib, unsigned T) {
    Mirror m;
    const bool have = lib && m.load(lib, f);
    if (lib && !have && f != kAcos) return 2;
    std::vector<Table> tabs(T);
    std::vector<uint64_t> bad(T, 0);
    std::vector<std::vector<Diff>> diffs(T);
    on_threads(T, [&](unsigned t) {
        subset(f, t, T, [&](uint64_t n) {
            float a, b;
            if (!gen(f, n, &a, &b)) return;
            uint32_t o[2];
            eval(f, a, b, o);
            Acc k;
            acc_init(k);
            measure(f, n, a, b, o, k);
            tabs[t].add(f, n, k);
            if (have && mirrored(f, a)) {
                uint32_t w[2];
                m.eval(a, b, w);
                if (!same_token(w, o) && bad[t]++ < 8) diffs[t].push_back({n, {w[0], w[1]}, {o[0], o[1]}});
            }
        });
    });
    Table all;
    uint64_t total = 0;
    std::vector<Diff> first;
    for (unsigned t = 0; t < T; ++t) {
        all.merge(tabs[t]);
        total += bad[t];
        first.insert(first.end(), diffs[t].begin(), diffs[t].end());
    }
    print_table(f, all, "host libm f64");
    if (have) {
        printf("oracle mismatches %llu\n", (unsigned long long)total);
        print_diffs(f, first, "oracle", "header");
    } else {
        printf("oracle mismatches none (no exported mirror)\n");
    }
    return total == 0 ? 0 : 1;
}

int main(int argc, char** argv) {
    int f = -1;
    bool host = false, no_device = false;
    const char* lib = nullptr;
    uint64_t mutate = kNoMutate, part = 0, parts = 1;
    unsigned T = 16;
    for (int i = 1; i < argc; ++i) {
        const std::string s = argv[i];
        if (s == "--host") host = true;
        else if (s == "--no-device") no_device = true;
        else if (s == "--oracle" && i + 1 < argc) lib = argv[++i];
        else if (s == "--mutate" && i + 1 < argc) mutate = strtoull(argv[++i], nullptr, 0);
        else if (s == "--threads" && i + 1 < argc) T = (unsigned)atoi(argv[++i]);
        else if (s == "--part" && i + 2 < argc) part = strtoull(argv[i + 1], nullptr, 0), parts = strtoull(argv[i + 2], nullptr, 0), i += 2;
        else {
            for (int k = 0; k < kFnCount; ++k)
                if (s == kFnName[k]) f = k;
            if (f < 0) break;
        }
    }
    T = std::min(std::max(T, 1u), 16u);
    if (f < 0 || parts == 0 || part >= parts) {
        fprintf(stderr, "usage: %s FUNC [--part K N] [--oracle LIB] [--mutate INDEX] [--no-device] | FUNC --host "
                        "[--oracle LIB] [--threads T]\n", argv[0]);
        return 2;
    }
    if (host) return run_host(f, lib, T);
    const uint64_t chunks = total_inputs(f) / kChunk;
    const uint64_t c0 = chunks * part / parts, c1 = chunks * (part + 1) / parts;
    Mirror m;
    const bool have = lib != nullptr && f != kAcos;  // acosf_ has no exported mirror
    if (have && !m.load(lib, f)) return 2;
    // the host's digests (while the kernel runs), and the header against the mirror
    const uint64_t nc = c1 - c0;
    std::vector<uint64_t> hd(nc);
    std::vector<uint64_t> obad(T, 0);
    std::vector<std::vector<Diff>> odiffs(T);
    auto host_pass = [&](unsigned t) {
        for (uint64_t c = t; c < nc; c += T) {
            uint64_t d = 0;
            for (uint64_t i = 0; i < kChunk; ++i) {
                const uint64_t n = (c0 + c) * kChunk + i;
                float a, b;
                if (!gen(f, n, &a, &b)) continue;
                uint32_t o[2];
                eval(f, a, b, o);
                d += digest_term(n, o);
                if (have && mirrored(f, a)) {
                    uint32_t w[2];
                    m.eval(a, b, w);
                    if (!same_token(w, o) && obad[t]++ < 8) odiffs[t].push_back({n, {w[0], w[1]}, {o[0], o[1]}});
                }
            }
            hd[c] = d;
        }
    };
    auto oracle_report = [&]() -> uint64_t {
        if (!have) {
            if (lib) printf("oracle mismatches none (no exported mirror)\n");
            return 0;
        }
        uint64_t total = 0;
        std::vector<Diff> first;
        for (unsigned t = 0; t < T; ++t) {
            total += obad[t];
            first.insert(first.end(), odiffs[t].begin(), odiffs[t].end());
        }
        std::sort(first.begin(), first.end(), [](const Diff& p, const Diff& q) { return p.n < q.n; });
        printf("oracle mismatches %llu\n", (unsigned long long)total);
        print_diffs(f, first, "oracle", "header");
        return total;
    };
    printf("function %s inputs 0x%llx..0x%llx\n", kFnName[f], (unsigned long long)(c0 * kChunk),
           (unsigned long long)(c1 * kChunk));
    if (no_device) {
        on_threads(T, host_pass);
        return oracle_report() == 0 ? 0 : 1;
    }
#if defined(__HIP__)
    Acc* dout = nullptr;
    uint32_t* ddump = nullptr;
    if (hipMalloc(&dout, nc * sizeof(Acc)) != hipSuccess || hipMalloc(&ddump, kChunk * 8) != hipSuccess) return 2;
    kSweep[f](c0, c1, mutate, dout);
    on_threads(T, host_pass);
    std::vector<Acc> dev(nc);
    if (hipMemcpy(dev.data(), dout, nc * sizeof(Acc), hipMemcpyDeviceToHost) != hipSuccess) {
        fprintf(stderr, "sweep failed: %s\n", hipGetErrorString(hipGetLastError()));
        return 2;
    }
    Table tab;
    uint64_t bad = 0;
    std::vector<Diff> first;
    std::vector<uint32_t> bits(2 * kChunk);
    for (uint64_t c = 0; c < nc; ++c) {
        tab.add(f, (c0 + c) * kChunk, dev[c]);
        if (dev[c].digest == hd[c]) continue;
        if (first.size() >= 8) {  // enough examples: count the chunk as one
            ++bad;
            continue;
        }
        kDump[f](c0 + c, mutate, ddump);
        if (hipMemcpy(bits.data(), ddump, kChunk * 8, hipMemcpyDeviceToHost) != hipSuccess) return 2;
        uint64_t in_chunk = 0;
        for (uint64_t i = 0; i < kChunk; ++i) {
            const uint64_t n = (c0 + c) * kChunk + i;
            float a, b;
            if (!gen(f, n, &a, &b)) continue;
            uint32_t o[2];
            eval(f, a, b, o);
            if (!same_token(o, &bits[2 * i])) {
                ++in_chunk;
                if (first.size() < 8) first.push_back({n, {o[0], o[1]}, {bits[2 * i], bits[2 * i + 1]}});
            }
        }
        bad += in_chunk ? in_chunk : 1;  // a digest that differs with no differing input is still a failure
    }
    print_table(f, tab, "device f64 library");
    printf("mismatches %llu\n", (unsigned long long)bad);
    print_diffs(f, first, "host", "device");
    const uint64_t obad_total = oracle_report();
    (void)hipFree(dout);
    (void)hipFree(ddump);
    return bad == 0 && obad_total == 0 ? 0 : 1;
#else
    (void)mutate;
    fprintf(stderr, "this build has no GPU side: use --host\n");
    return 2;
#endif
}
