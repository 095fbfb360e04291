// gu_probe.hip -- the float64 building blocks of gu_softmax.hpp evaluated on the caller's arrays, one lane per item (include/gu_diag.h:
// gu_probe_numeric, gu_probe_numeric_softmax).  The kernels call the very functions the learner kernels inline -- gu_exp, gu_recip14,
// gu_is_recip, gu_softmax_row, gu_softmax_action -- so the tests can put them on arguments that learning never reaches and compare
// with exact arithmetic.  They read and write the engine's scratch only: no table, no env state, no carry is touched.
#include "gu_softmax.hpp"

#define GU_PROBE_BLOCK 256

__global__ void __launch_bounds__(GU_PROBE_BLOCK) gu_probe_unary_kernel(int32_t op, int64_t n, const double *__restrict__ x, double *__restrict__ y)
{
    const int64_t i = (int64_t)blockIdx.x * GU_PROBE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    y[i] = op == GU_PROBE_EXP ? gu_exp(v) : op == GU_PROBE_RECIP14 ? gu_recip14(v) : gu_is_recip(v);
}

__global__ void __launch_bounds__(GU_PROBE_BLOCK) gu_probe_softmax_kernel(int64_t n, const double *__restrict__ pref, const uint32_t *__restrict__ w,
                                                                          double *__restrict__ e, double *__restrict__ Z, double *__restrict__ iz,
                                                                          int32_t *__restrict__ action)
{
    const int64_t i = (int64_t)blockIdx.x * GU_PROBE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const SoftRow s = gu_softmax_row(gu_q_load(pref + i * 4));
    e[i * 4 + 0] = s.e0;
    e[i * 4 + 1] = s.e1;
    e[i * 4 + 2] = s.e2;
    e[i * 4 + 3] = s.e3;
    Z[i] = s.Z;
    iz[i] = gu_recip14(s.Z);
    action[i] = (int32_t)gu_softmax_action(s, w[i]);
}

static unsigned gu_probe_blocks(int64_t n)
{
    return (unsigned)((n + GU_PROBE_BLOCK - 1) / GU_PROBE_BLOCK);
}

extern "C" {

int gu_probe_numeric(gu_handle h, int32_t op, int64_t n, const double *x, double *y)
{
    GU_ENTER(h);
    GU_REQUIRE(op == GU_PROBE_EXP || op == GU_PROBE_RECIP14 || op == GU_PROBE_IS_RECIP, GU_ERR_INVALID, "unknown probe %d", (int)op);
    GU_REQUIRE(x != nullptr && y != nullptr, GU_ERR_INVALID, "x or y is NULL");
    GU_REQUIRE(n >= 0 && n <= GU_PROBE_MAX, GU_ERR_INVALID, "n %lld out of range (0 .. %lld)", (long long)n, (long long)GU_PROBE_MAX);
    if (n == 0) return GU_OK;
    const size_t bytes = (size_t)n * sizeof(double);
    GU_TRY(gu_ensure_scratch(h, 2 * bytes));
    double *dx = reinterpret_cast<double *>(h->d_scratch), *dy = dx + n;
    GU_HIP(hipMemcpyAsync(dx, x, bytes, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(gu_probe_unary_kernel, dim3(gu_probe_blocks(n)), dim3(GU_PROBE_BLOCK), 0, h->stream, op, n, dx, dy);
    GU_HIP(hipGetLastError());
    GU_HIP(hipMemcpyAsync(y, dy, bytes, hipMemcpyDeviceToHost, h->stream));
    GU_HIP(hipStreamSynchronize(h->stream));
    return GU_OK;
}

int gu_probe_numeric_softmax(gu_handle h, int64_t n, const double *pref, const uint32_t *w, double *e, double *Z, double *iz, int32_t *action)
{
    GU_ENTER(h);
    GU_REQUIRE(pref != nullptr && w != nullptr, GU_ERR_INVALID, "pref or w is NULL");
    GU_REQUIRE(e != nullptr && Z != nullptr && iz != nullptr && action != nullptr, GU_ERR_INVALID, "e, Z, iz or action is NULL");
    GU_REQUIRE(n >= 0 && n <= GU_PROBE_MAX, GU_ERR_INVALID, "n %lld out of range (0 .. %lld)", (long long)n, (long long)GU_PROBE_MAX);
    if (n == 0) return GU_OK;
    // scratch: pref [n][4] | e [n][4] | Z [n] | iz [n] | w [n] | action [n] -- 88 n bytes, the doubles first (16-byte rows stay aligned)
    const size_t un = (size_t)n;
    GU_TRY(gu_ensure_scratch(h, un * 88));
    double *d_pref = reinterpret_cast<double *>(h->d_scratch), *d_e = d_pref + un * 4, *d_Z = d_e + un * 4, *d_iz = d_Z + un;
    uint32_t *d_w = reinterpret_cast<uint32_t *>(d_iz + un);
    int32_t *d_a = reinterpret_cast<int32_t *>(d_w + un);
    GU_HIP(hipMemcpyAsync(d_pref, pref, un * 32, hipMemcpyHostToDevice, h->stream));
    GU_HIP(hipMemcpyAsync(d_w, w, un * 4, hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(gu_probe_softmax_kernel, dim3(gu_probe_blocks(n)), dim3(GU_PROBE_BLOCK), 0, h->stream, n, d_pref, d_w, d_e, d_Z, d_iz, d_a);
    GU_HIP(hipGetLastError());
    GU_HIP(hipMemcpyAsync(e, d_e, un * 32, hipMemcpyDeviceToHost, h->stream));
    GU_HIP(hipMemcpyAsync(Z, d_Z, un * 8, hipMemcpyDeviceToHost, h->stream));
    GU_HIP(hipMemcpyAsync(iz, d_iz, un * 8, hipMemcpyDeviceToHost, h->stream));
    GU_HIP(hipMemcpyAsync(action, d_a, un * 4, hipMemcpyDeviceToHost, h->stream));
    GU_HIP(hipStreamSynchronize(h->stream));
    return GU_OK;
}

}  // extern "C"
