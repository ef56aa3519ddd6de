// vq_common.inc -- constants, error strings, the kernel-launch helper, metric / padded-dim dispatch, packed (value, index) keys.
// Included by vq_kernels.hip inside its anonymous namespace (single translation unit).

// (kTileCodes, kPackSlack, padded_dim, round_up, sub_tiles: vq_search_plan.h, shared with the launch plans)
constexpr int kModeFused = 0;
constexpr int kModeKeys = 1;      // packed keys, atomic MIN into ONE plane (the caller initialised it)
constexpr int kModeKeyParts = 2;  // packed keys, plain stores: K split z writes plane z (no init, no atomics)

// (the error string is shared by all parts of a split build -- see "Build parts" in vq_kernels.hip -- so it lives in the
//  named namespace; everything else in this file has internal linkage)
}  // namespace
namespace vqi {
extern thread_local char g_err[512];
}
namespace {
using vqi::g_err;

int fail(int code, const char *msg) {
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

int fail(int code, const char *who, const char *msg) {
    snprintf(g_err, sizeof(g_err), "%s: %s", who, msg);
    return code;
}

int hip_fail(hipError_t e, const char *what) {
    snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
    return (int)e;
}

// The one kernel launch of the library: raise the kernel's dynamic-LDS limit first when the launcher asks for it (BIG_LDS),
// launch, check.  `what` names the launch in the error string.  hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a
// per-device property of a kernel, so the "already raised" flags are per kernel (Kern is a template ARGUMENT: kernels of one
// signature, such as every vq_search_mfma<..>, must not share them), per thread and per device ordinal -- a process that
// drives several GPUs raises the limit on each of them.
constexpr int kMaxDevices = 64;
constexpr bool kBigLds = true;

template <auto Kern, bool BIG_LDS = false, typename... A>
int launch(dim3 grid, dim3 block, size_t lds, hipStream_t s, const char *what, const A &...args) {
    if constexpr (BIG_LDS) {
        static thread_local bool raised[kMaxDevices] = {};
        int dev = -1;
        if (hipGetDevice(&dev) != hipSuccess) return fail(VQ_E_NODEVICE, "vq: no HIP device");
        const bool tracked = dev >= 0 && dev < kMaxDevices;
        if (!tracked || !raised[dev]) {
            hipError_t e = hipFuncSetAttribute((const void *)Kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (e != hipSuccess) return hip_fail(e, "hipFuncSetAttribute");
            if (tracked) raised[dev] = true;
        }
    }
    hipLaunchKernelGGL(Kern, grid, block, lds, s, args...);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : hip_fail(e, what);
}

// run-time value -> template argument: f is called with a std::integral_constant and returns the launch's status
template <typename F>
int with_metric(int metric, F f) {
    if (metric == VQ_METRIC_EUCLID) return f(std::integral_constant<int, VQ_METRIC_EUCLID>{});
    return f(std::integral_constant<int, VQ_METRIC_DOT>{});
}

template <typename F, typename U>
int with_padded_dim(int DP, F f, U on_unsupported) {
    switch (DP) {
        case 32: return f(std::integral_constant<int, 32>{});
        case 64: return f(std::integral_constant<int, 64>{});
        case 128: return f(std::integral_constant<int, 128>{});
        case 256: return f(std::integral_constant<int, 256>{});
        case 512: return f(std::integral_constant<int, 512>{});
    }
    return on_unsupported();
}

// ------------------------------------------------------------------------------------------------
// packed (value, index) keys: signed 64-bit, MIN wins, lowest index on equal values
// ------------------------------------------------------------------------------------------------
// A NaN similarity is argmax's maximum (ATen, utils/general.py:128), so a NaN value is the BEST key of either metric and the
// lowest index wins among NaNs: Euclid m = 0 for NaN and 1 + bits otherwise; dot: NaN canonicalised to the positive quiet
// NaN, which the order-preserving map already places above +inf.
template <int METRIC>
__device__ __forceinline__ long long make_key(float v, long long idx) {
    unsigned b = __float_as_uint(v);
    const bool nan = v != v;
    unsigned m;
    if (METRIC == VQ_METRIC_DOT) {
        if (nan) b = 0x7FC00000u;
        unsigned mono = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
        m = ~mono;
    } else {
        m = nan ? 0u : b + 1u;  // sqrt distance >= 0: IEEE bits are order preserving
    }
    return (long long)(((unsigned long long)(m ^ 0x80000000u) << 32) | (unsigned long long)(unsigned)idx);
}

__device__ __forceinline__ float key_value(long long key, int metric) {
    unsigned m = (unsigned)((unsigned long long)key >> 32) ^ 0x80000000u;
    unsigned b;
    if (metric == VQ_METRIC_DOT) {
        unsigned mono = ~m;
        b = (mono & 0x80000000u) ? (mono ^ 0x80000000u) : ~mono;
    } else {
        b = m ? m - 1u : 0x7FC00000u;
    }
    return __uint_as_float(b);
}

