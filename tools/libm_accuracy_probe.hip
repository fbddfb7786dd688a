// Accuracy of the device rsqrtf / cosf / sinf that norm.hip calls, against float64 on the host.  tests/util_norm_ref.py takes its
// rho (rsqrtf, relative) and a (cosf / sinf, absolute) from this program's output (profiles/libm_accuracy_gfx950.txt): twice the
// worst value printed here.  Built with the flags of bagel_amd/build.py:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off tools/libm_accuracy_probe.hip -o libm_accuracy_probe
//   ./libm_accuracy_probe > profiles/libm_accuracy_gfx950.txt
// Arguments: rsqrtf over the values ss / n + eps takes (bit patterns evenly spread over [2^-30, 2^20], 2^22 of them);
// cosf / sinf over (a) bit patterns evenly spread over [2^-24, 32768], 2^22 of them, (b) 2^22 evenly spaced angles in [0, 32768],
// (c) the angles fl32(pos * inv_freq) the tables use: every position 0 .. 32767 times the inv_freq of head dims 32, 72, 128.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#define CK(x)                                                                            \
    do {                                                                                 \
        hipError_t e_ = (x);                                                             \
        if (e_ != hipSuccess) {                                                          \
            std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));                 \
            return 1;                                                                    \
        }                                                                                \
    } while (0)

__global__ void eval_kernel(const float* __restrict__ x, float* __restrict__ r, float* __restrict__ c, float* __restrict__ s, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    r[i] = rsqrtf(x[i]);
    c[i] = cosf(x[i]);
    s[i] = sinf(x[i]);
}

static float from_bits(unsigned u) { float f; std::memcpy(&f, &u, 4); return f; }
static unsigned to_bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }
static double ulp32(double v) {   // spacing of fp32 at |v| (normal range)
    int e;
    std::frexp(std::fabs(v), &e);
    return std::ldexp(1.0, e - 24);
}

struct Worst { double rel = 0, abs_ = 0, ulps = 0; float at_rel = 0, at_abs = 0; };
static void note(Worst& w, float arg, double got, double want) {
    const double d = std::fabs(got - want);
    if (d > w.abs_) { w.abs_ = d; w.at_abs = arg; }
    if (want != 0 && d / std::fabs(want) > w.rel) { w.rel = d / std::fabs(want); w.at_rel = arg; }
    if (want != 0 && d / ulp32(want) > w.ulps) w.ulps = d / ulp32(want);
}

static int run(const char* name, const std::vector<float>& x, bool do_rsqrt, bool do_trig) {
    const long n = (long)x.size();
    float *dx, *dr, *dc, *ds;
    CK(hipMalloc(&dx, n * 4)); CK(hipMalloc(&dr, n * 4)); CK(hipMalloc(&dc, n * 4)); CK(hipMalloc(&ds, n * 4));
    CK(hipMemcpy(dx, x.data(), n * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, dx, dr, dc, ds, n);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<float> r(n), c(n), s(n);
    CK(hipMemcpy(r.data(), dr, n * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(c.data(), dc, n * 4, hipMemcpyDeviceToHost));
    CK(hipMemcpy(s.data(), ds, n * 4, hipMemcpyDeviceToHost));
    CK(hipFree(dx)); CK(hipFree(dr)); CK(hipFree(dc)); CK(hipFree(ds));
    Worst wr, wc, ws;
    for (long i = 0; i < n; ++i) {
        const double a = (double)x[i];
        if (do_rsqrt) note(wr, x[i], (double)r[i], 1.0 / std::sqrt(a));
        if (do_trig) { note(wc, x[i], (double)c[i], std::cos(a)); note(ws, x[i], (double)s[i], std::sin(a)); }
    }
    if (do_rsqrt)
        std::printf("rsqrtf %-28s n=%ld  worst relative error %.4g = %.3f * 2^-24 (at %.9g)  worst ulp %.3f\n", name, n, wr.rel,
                    wr.rel * 16777216.0, wr.at_rel, wr.ulps);
    if (do_trig) {
        std::printf("cosf   %-28s n=%ld  worst absolute error %.4g = %.3f * 2^-24 (at %.9g)  worst ulp of the result %.3f\n", name, n,
                    wc.abs_, wc.abs_ * 16777216.0, wc.at_abs, wc.ulps);
        std::printf("sinf   %-28s n=%ld  worst absolute error %.4g = %.3f * 2^-24 (at %.9g)  worst ulp of the result %.3f\n", name, n,
                    ws.abs_, ws.abs_ * 16777216.0, ws.at_abs, ws.ulps);
    }
    return 0;
}

static std::vector<float> bit_spread(float lo, float hi, long n) {
    const unsigned a = to_bits(lo), b = to_bits(hi);
    std::vector<float> v(n);
    for (long i = 0; i < n; ++i) v[i] = from_bits(a + (unsigned)(((unsigned long long)(b - a) * (unsigned long long)i) / (unsigned long long)(n - 1)));
    return v;
}

int main() {
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    std::printf("# device %s (%s); flags -O3 -ffp-contract=off; reference: float64 libm on the host\n", prop.name, prop.gcnArchName);
    const long N = 1L << 22;
    if (run("bits [2^-30, 2^20]", bit_spread(std::ldexp(1.0f, -30), std::ldexp(1.0f, 20), N), true, false)) return 1;
    if (run("bits [2^-24, 32768]", bit_spread(std::ldexp(1.0f, -24), 32768.0f, N), false, true)) return 1;
    {
        std::vector<float> v(N);
        for (long i = 0; i < N; ++i) v[i] = (float)(32768.0 * (double)i / (double)(N - 1));
        if (run("linear [0, 32768]", v, false, true)) return 1;
    }
    const int hds[3] = {32, 72, 128};
    const double bases[3] = {1e6, 1e4, 1e6};
    for (int k = 0; k < 3; ++k) {
        const int hd = hds[k], half = hd / 2;
        std::vector<float> v;
        v.reserve((size_t)32768 * half);
        for (int p = 0; p < 32768; ++p)
            for (int c = 0; c < half; ++c) {
                const float inv = 1.0f / std::pow((float)bases[k], (float)(2 * c) / (float)hd);
                v.push_back((float)p * inv);
            }
        char name[64];
        std::snprintf(name, sizeof name, "pos * inv_freq, hd %d base %.0e", hd, bases[k]);
        if (run(name, v, false, true)) return 1;
    }
    return 0;
}
