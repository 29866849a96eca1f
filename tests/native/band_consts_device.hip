// The f64 band's frame constants and step on the device against the host
// build of the same header (geo_band.h), by bytes:
//  * geo::band_consts_into, one lane per case, into a zero-filled BandConsts in
//    global memory (a batched GEO_FLAG_RING_F64 launch derives them so; f64
//    sqrt and divide must round as the host's), and geo::band_kx: 8192 cases
//    of fixed-seed frames and scenes with the edges of every branch: psi 0 and
//    +-(1 - 2^-24), identity and rotated movement_to_central, r_obs the f32
//    next above rs, exactly 3 rs / 2 and its f32 neighbours, sphere_r on
//    either side of 3 rs / 2 and of r_obs and equal to each;
//  * geo::min64_ (an inline-asm v_min_f64 on the device) against the host's
//    min64_ and against fmin on all ordered pairs of 72 values: +-0,
//    denormals, +-1, +-inf, quiet NaNs of both signs, random finite doubles
//    (any NaN result is one token; of +0 and -0, where C leaves fmin's choice
//    open, IEEE 754-2019 minimumNumber's -0 is required);
//  * geo::band_rk4 on 2^16 random states and steps, its constants formed as
//    band_steps forms Newton's.
// Prints the first differing field of the first differing cases and
// "mismatches N"; exit status 0 iff N == 0.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../schwarzschild_raytracer_wgpu_amd/csrc/geo_band.h"

struct Case {
    geo_frame f;
    float rs, sphere_r, r_obs, step;
    uint32_t max_steps, width, height;
};
struct Rk4In {
    double U, V, h;
};
struct Rk4Out {
    double NU, NV;
};

__host__ __device__ inline void run_case(const Case& c, geo::BandConsts& k, float& kx) {
    geo::band_consts_into(k, c.f, c.rs, c.sphere_r, c.r_obs, c.step, c.max_steps, c.width, c.height);
    kx = geo::band_kx(c.rs, c.r_obs);
}
__host__ __device__ inline Rk4Out run_rk4(const Rk4In& s) {
    const double ns = s.h, n2 = ns * ns;
    Rk4Out o;
    geo::band_rk4(s.U, s.V, ns, ns / 2.0, n2 / 4.0, n2 / 2.0, ns / 6.0, n2 / 6.0, &o.NU, &o.NV);
    return o;
}

__global__ __launch_bounds__(256) void consts_kernel(const Case* cs, geo::BandConsts* out, float* kx, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) run_case(cs[i], out[i], kx[i]);
}
__global__ __launch_bounds__(256) void min_kernel(const double* v, double* out, uint32_t nv) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < nv * nv) out[i] = geo::min64_(v[i / nv], v[i % nv]);
}
__global__ __launch_bounds__(256) void rk4_kernel(const Rk4In* in, Rk4Out* out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = run_rk4(in[i]);
}

static uint64_t g_state = 0x5eed5eed2024ull;
static uint64_t next_u64() {  // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static double uni() { return (double)(next_u64() >> 11) * 0x1p-53; }  // [0, 1)
static double uni(double lo, double hi) { return lo + (hi - lo) * uni(); }
static double log_uni(double lo, double hi) { return lo * std::exp(std::log(hi / lo) * uni()); }

static Case make_case(uint32_t i) {
    static const uint32_t kSteps[4] = {1u, 3u, 2048u, (1u << 24) - 1u};
    static const uint32_t kSizes[6] = {1u, 2u, 36u, 64u, 3840u, 7680u};
    Case c;
    std::memset(&c, 0, sizeof c);
    for (int j = 0; j < 16; ++j) c.f.display_to_movement[j] = (float)uni(-4.0, 4.0);
    float* m = c.f.movement_to_central;
    m[0] = m[5] = m[10] = m[15] = 1.0f;
    if (i & 1u) {  // a random rotation (from a unit quaternion)
        double q[4], n2 = 0.0;
        for (double& x : q) x = uni(-1.0, 1.0), n2 += x * x;
        for (double& x : q) x /= std::sqrt(n2);
        const double w = q[0], x = q[1], y = q[2], z = q[3];
        m[0] = (float)(1 - 2 * (y * y + z * z)), m[1] = (float)(2 * (x * y + z * w)), m[2] = (float)(2 * (x * z - y * w));
        m[4] = (float)(2 * (x * y - z * w)), m[5] = (float)(1 - 2 * (x * x + z * z)), m[6] = (float)(2 * (y * z + x * w));
        m[8] = (float)(2 * (x * z + y * w)), m[9] = (float)(2 * (y * z - x * w)), m[10] = (float)(1 - 2 * (x * x + y * y));
    }
    for (int j = 0; j < 16; ++j) c.f.central_to_uv[j] = (float)uni(-1.0, 1.0);
    const uint32_t pk = (i >> 1) & 7u;
    c.f.psi_factor_and_position[0] = pk == 0 ? 0.0f : pk == 1 ? 1.0f - 0x1p-24f : pk == 2 ? -(1.0f - 0x1p-24f) : (float)uni(-0.999, 0.999);
    for (int j = 1; j < 4; ++j) c.f.psi_factor_and_position[j] = (float)uni(-50.0, 50.0);
    c.rs = (float)uni(0.25, 4.0);
    c.r_obs = (float)(c.rs * log_uni(1.0 + 0x1p-23, 300.0));
    switch ((i >> 4) & 7u) {
        case 0: c.r_obs = std::nextafterf(c.rs, INFINITY); break;
        case 1: c.rs = 2.0f, c.r_obs = 3.0f; break;
        case 2: c.rs = 2.0f, c.r_obs = std::nextafterf(3.0f, 4.0f); break;
        case 3: c.rs = 2.0f, c.r_obs = std::nextafterf(3.0f, 0.0f); break;
        default: break;
    }
    if (!(c.r_obs > c.rs)) c.r_obs = std::nextafterf(c.rs, INFINITY);
    const float r32 = 1.5f * c.rs;
    switch ((i >> 7) % 7u) {
        case 0: c.sphere_r = r32 * 0.9f; break;
        case 1: c.sphere_r = r32 * 1.1f; break;
        case 2: c.sphere_r = r32; break;
        case 3: c.sphere_r = c.r_obs * 0.9f; break;
        case 4: c.sphere_r = c.r_obs * 1.1f; break;
        case 5: c.sphere_r = c.r_obs; break;
        default: c.sphere_r = (float)(c.rs * log_uni(0.5, 400.0)); break;
    }
    c.step = (float)log_uni(0.005, 3.0);
    c.max_steps = kSteps[next_u64() % 4u];
    c.width = kSizes[next_u64() % 6u];
    c.height = kSizes[next_u64() % 6u];
    return c;
}

struct Field {
    const char* name;
    size_t off, size;
};
#define BC_FIELD(x) {#x, offsetof(geo::BandConsts, x), sizeof(((geo::BandConsts*)nullptr)->x)}
static const Field kFields[] = {
    BC_FIELD(a), BC_FIELD(b), BC_FIELD(c), BC_FIELD(m1), BC_FIELD(k), BC_FIELD(kt), BC_FIELD(r), BC_FIELD(energy),
    BC_FIELD(hor), BC_FIELD(barrier_lim), BC_FIELD(radial_falling), BC_FIELD(radial_outgoing), BC_FIELD(scale),
    BC_FIELD(U0), BC_FIELD(SU), BC_FIELD(BD), BC_FIELD(HU), BC_FIELD(lo), BC_FIELD(hi), BC_FIELD(h), BC_FIELD(hh),
    BC_FIELD(hh2), BC_FIELD(hhh), BC_FIELD(h6), BC_FIELD(h2_6), BC_FIELD(kx), BC_FIELD(max_steps), BC_FIELD(above0),
    BC_FIELD(pf_always), BC_FIELD(pf_falling), BC_FIELD(pf_outgoing), BC_FIELD(m1_identity)};

static const char* first_field(const geo::BandConsts& p, const geo::BandConsts& q) {
    for (const Field& f : kFields)
        if (std::memcmp((const char*)&p + f.off, (const char*)&q + f.off, f.size) != 0) return f.name;
    return "padding";
}

static uint64_t token(double x) {
    uint64_t b;
    std::memcpy(&b, &x, 8);
    return x != x ? 0x7ff8000000000000ull : b;
}

#define HIP_OK(e)                                                             \
    do {                                                                      \
        const hipError_t err_ = (e);                                          \
        if (err_ != hipSuccess) {                                             \
            fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(err_));         \
            return 2;                                                         \
        }                                                                     \
    } while (0)

int main() {
    unsigned long long bad = 0;
    int shown = 0;

    // ---- band_consts_into and band_kx ----
    const uint32_t n = 8192;
    std::vector<Case> cases(n);
    for (uint32_t i = 0; i < n; ++i) cases[i] = make_case(i);
    Case* dc;
    geo::BandConsts* dk;
    float* dkx;
    HIP_OK(hipMalloc(&dc, n * sizeof(Case)));
    HIP_OK(hipMalloc(&dk, n * sizeof(geo::BandConsts)));
    HIP_OK(hipMalloc(&dkx, n * sizeof(float)));
    HIP_OK(hipMemcpy(dc, cases.data(), n * sizeof(Case), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dk, 0, n * sizeof(geo::BandConsts)));
    HIP_OK(hipMemset(dkx, 0, n * sizeof(float)));
    hipLaunchKernelGGL(consts_kernel, dim3((n + 255u) / 256u), dim3(256), 0, 0, dc, dk, dkx, n);
    std::vector<geo::BandConsts> gk(n);
    std::vector<float> gkx(n);
    HIP_OK(hipMemcpy((void*)gk.data(), dk, n * sizeof(geo::BandConsts), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(gkx.data(), dkx, n * sizeof(float), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < n; ++i) {
        geo::BandConsts hk;
        std::memset((void*)&hk, 0, sizeof hk);
        float hkx = 0.0f;
        run_case(cases[i], hk, hkx);
        const bool dk_bad = std::memcmp((const void*)&hk, (const void*)&gk[i], sizeof hk) != 0;
        const bool kx_bad = std::memcmp(&hkx, &gkx[i], 4) != 0;
        if (dk_bad || kx_bad) {
            ++bad;
            if (shown++ < 8)
                printf("  case %u (rs %.9g sphere_r %.9g r_obs %.9g step %.9g psi %.9g %ux%u): %s differs\n", i,
                       cases[i].rs, cases[i].sphere_r, cases[i].r_obs, cases[i].step,
                       cases[i].f.psi_factor_and_position[0], cases[i].width, cases[i].height,
                       dk_bad ? first_field(hk, gk[i]) : "band_kx");
        }
    }
    printf("band_consts_into, band_kx: %u cases\n", n);

    // ---- min64_ ----
    std::vector<double> v = {0.0, -0.0, 4.9406564584124654e-324, -4.9406564584124654e-324, 2.2250738585072009e-308,
                             -2.2250738585072009e-308, 1.0, -1.0, (double)INFINITY, -(double)INFINITY,
                             std::nan(""), -std::nan(""), 2.2250738585072014e-308, 1.7976931348623157e308};
    while (v.size() < 72) {
        uint64_t b = next_u64();
        if (((b >> 52) & 0x7ffu) == 0x7ffu) b &= ~(1ull << 62);  // finite
        double x;
        std::memcpy(&x, &b, 8);
        v.push_back(x);
    }
    const uint32_t nv = (uint32_t)v.size();
    double *dv, *dm;
    HIP_OK(hipMalloc(&dv, nv * 8));
    HIP_OK(hipMalloc(&dm, (size_t)nv * nv * 8));
    HIP_OK(hipMemcpy(dv, v.data(), nv * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dm, 0, (size_t)nv * nv * 8));
    hipLaunchKernelGGL(min_kernel, dim3((nv * nv + 255u) / 256u), dim3(256), 0, 0, dv, dm, nv);
    std::vector<double> gm((size_t)nv * nv);
    HIP_OK(hipMemcpy(gm.data(), dm, gm.size() * 8, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < nv * nv; ++i) {
        const double p = v[i / nv], q = v[i % nv];
        const double want = geo::min64_(p, q);
        // fmin of zeros of opposite sign: C allows either; IEEE 754-2019 minimumNumber says -0
        const bool open = p == 0.0 && q == 0.0 && std::signbit(p) != std::signbit(q);
        const double lib = open ? -0.0 : std::fmin(p, q);
        if (token(want) != token(gm[i]) || token(lib) != token(gm[i])) {
            ++bad;
            if (shown++ < 8)
                printf("  min64_(%a, %a): host %a (0x%016llx), fmin %a, device %a (0x%016llx)\n", p, q, want,
                       (unsigned long long)token(want), lib, gm[i], (unsigned long long)token(gm[i]));
        }
    }
    printf("min64_: %u pairs\n", nv * nv);

    // ---- band_rk4 ----
    const uint32_t nr = 1u << 16;
    std::vector<Rk4In> rin(nr);
    for (Rk4In& s : rin) s.U = uni(-4.0, 4.0), s.V = uni(-4.0, 4.0), s.h = log_uni(1e-3, 3.0);
    Rk4In* dri;
    Rk4Out* dro;
    HIP_OK(hipMalloc(&dri, nr * sizeof(Rk4In)));
    HIP_OK(hipMalloc(&dro, nr * sizeof(Rk4Out)));
    HIP_OK(hipMemcpy(dri, rin.data(), nr * sizeof(Rk4In), hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dro, 0, nr * sizeof(Rk4Out)));
    hipLaunchKernelGGL(rk4_kernel, dim3((nr + 255u) / 256u), dim3(256), 0, 0, dri, dro, nr);
    std::vector<Rk4Out> gro(nr);
    HIP_OK(hipMemcpy(gro.data(), dro, nr * sizeof(Rk4Out), hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < nr; ++i) {
        const Rk4Out want = run_rk4(rin[i]);
        if (token(want.NU) != token(gro[i].NU) || token(want.NV) != token(gro[i].NV)) {
            ++bad;
            if (shown++ < 8)
                printf("  band_rk4(U %a, V %a, h %a): host (%a, %a), device (%a, %a)\n", rin[i].U, rin[i].V, rin[i].h,
                       want.NU, want.NV, gro[i].NU, gro[i].NV);
        }
    }
    printf("band_rk4: %u states\n", nr);

    printf("mismatches %llu\n", bad);
    return bad == 0 ? 0 : 1;
}
