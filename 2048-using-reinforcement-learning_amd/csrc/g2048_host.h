// g2048_host.h -- the host side every entry point of the C-ABI shares: one error string, one way to check arguments and HIP
// calls, one way to pick a kernel instantiation from run-time values. Host code only, included by the library's .hip
// files and nothing else. An entry point reads: checks (fail / aligned), launch (with_* where the kernel is a template),
// return check_launch("<its name>").
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <cmath>
#include <type_traits>

#include "../../include/g2048.h"

namespace g2048 {

// ------------------------------------------------------------------------------------------------------------ errors --
inline thread_local char g_err[256] = "";           // what g2048_last_error() returns

__attribute__((format(printf, 2, 3))) inline int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

// a HIP call's status as the entry point's: "<entry point>: <hip error string>"
inline int check_hip(hipError_t e, const char *what)
{
    return e == hipSuccess ? G2048_OK : fail(G2048_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
}

inline int check_launch(const char *what) { return check_hip(hipGetLastError(), what); }

// ---------------------------------------------------------------------------------------------------------- arguments --
// bytes: a power of two. A null pointer is aligned, so an optional array needs no guard of its own.
inline bool aligned(const void *p, size_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) == 0; }

inline unsigned blocks_for(size_t n, size_t per_block) { return (unsigned)((n + per_block - 1) / per_block); }

inline bool good_precision(int p) { return p == G2048_POLICY_F32 || p == G2048_POLICY_BF16; }

// the encoder shapes the transformer policy and the Q-network are compiled for
inline bool good_encoder_shape(int dim_ff, int n_layers)
{
    return dim_ff >= 32 && dim_ff % 32 == 0 && dim_ff <= 65536 && n_layers >= 1 && n_layers <= 64;
}

// a loss coefficient or the clip range of the two PPO passes (g2048_ppo_grad.hip, g2048_tpolicy_grad_pass.h)
inline bool good_coef(float v) { return v >= 0.0f && std::isfinite(v); }

// ------------------------------------------------------- the two encoder networks (g2048_tpolicy.hip, g2048_qnet.hip) --
// precision and encoder shape: G2048_OK, or the error as `entry`'s. precision_arg: what that entry point calls the argument
// the precision arrives in ("precision", "opts (precision)")
inline int check_encoder_net(const char *entry, int precision, const char *precision_arg, int dim_ff, int n_layers)
{
    if (!good_precision(precision)) return fail(G2048_ERR_ARG, "%s: unknown %s", entry, precision_arg);
    if (!good_encoder_shape(dim_ff, n_layers))
        return fail(G2048_ERR_ARG, "%s: dim_ff must be a multiple of 32 (32 .. 65536) and n_layers 1 .. 64", entry);
    return G2048_OK;
}

// One launch of pack_matrix_kernel (g2048_mfma.h; `kernel` is its instantiation for the precision, `chunk` that precision's input
// features per fragment): the matrix of rows_a + rows_b rows (a over b) x K into the fragments from `dst` on, packed column
// k = plain column (k % inner) * stride + k / inner (the identity for inner = K, stride = 1).
template <class Kernel>
void launch_pack_matrix(Kernel kernel, int chunk, hipStream_t s, void *dst, const float *a, int rows_a, int K, int inner, int stride,
                        const float *b = nullptr, int rows_b = 0)
{
    const unsigned frags = (unsigned)(((rows_a + rows_b + 15) / 16) * (K / chunk));
    hipLaunchKernelGGL(kernel, dim3(frags), dim3(256), 0, s, a, rows_a, b, rows_b, K, inner, stride, frags * 256u, static_cast<uint32_t *>(dst));
}

// --------------------------------------------------------------------------------------- complete games of a network --
// What g2048_play_policy_games, g2048_play_tpolicy_games and g2048_play_qnet_games share on the host (the device side is
// g2048_play.h). `stem` is the entry point's name without "_games", e.g. "g2048_play_policy": the messages name
// <stem>_games and <stem>_workspace.

// the workspace is the ticket counter (uint64), padded
inline size_t ticket_workspace_bytes(size_t n_games)
{
    (void)n_games;
    return 64;
}

// the arguments the three entry points have in common: G2048_OK, or the error as the entry point's
inline int check_play_args(const char *stem, const void *boards, const uint32_t *score, const void *packed, const int32_t *moves,
                           const int32_t *valid, const int32_t *invalid, const int32_t *milestones, const double *reward_or_null,
                           const uint8_t *alive, int max_moves, size_t n_games, const void *workspace, size_t workspace_bytes)
{
    if (!boards || !score || !packed || !moves || !valid || !invalid || !milestones || !alive || !workspace)
        return fail(G2048_ERR_ARG, "%s_games: null pointer", stem);
    if (!aligned(boards, 16) || !aligned(packed, 16) || !aligned(milestones, 16) || !aligned(score, 4) || !aligned(moves, 4) ||
        !aligned(valid, 4) || !aligned(invalid, 4) || !aligned(reward_or_null, 8) || !aligned(workspace, 8))
        return fail(G2048_ERR_ARG, "%s_games: misaligned pointer (boards, weights, milestones: 16 bytes; rewards, workspace: 8; counters "
                                   "and scores: 4)", stem);
    if (max_moves < 1) return fail(G2048_ERR_ARG, "%s_games: max_moves must be at least 1", stem);
    if (workspace_bytes < ticket_workspace_bytes(n_games))
        return fail(G2048_ERR_ARG, "%s_games: workspace smaller than %s_workspace(n_games)", stem, stem);
    return G2048_OK;
}

// before the launch, on its stream: the ticket counter to zero, the action bytes (if asked for) to 0xFF
inline int reset_play_buffers(const char *stem, void *workspace, uint8_t *actions_or_null, size_t n_games, int max_moves, hipStream_t s)
{
    hipError_t e = hipMemsetAsync(workspace, 0, sizeof(unsigned long long), s);
    if (e == hipSuccess && actions_or_null) e = hipMemsetAsync(actions_or_null, 0xff, n_games * (size_t)max_moves, s);
    return e == hipSuccess ? G2048_OK : fail(G2048_ERR_HIP, "%s_games: hipMemsetAsync: %s", stem, hipGetErrorString(e));
}

// ------------------------------------------------------------------------------------------------------------ device --
constexpr int kFallbackCus = 256;                    // MI355X's compute-unit count, if the device cannot be asked

// asked per call: a partitioned or CU-masked device simply reports fewer
inline int device_cus()
{
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
        (void)hipGetLastError();
        return kFallbackCus;
    }
    return cus;
}

// blocks of `kernel` a compute unit holds at once (0: could not ask); x device_cus() = what the device holds
template <class Kernel>
int resident_per_cu(Kernel kernel, int block_threads)
{
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block_threads, 0) != hipSuccess || per_cu < 0) {
        (void)hipGetLastError();
        return 0;
    }
    return per_cu;
}

// ---------------------------------------------------------------------------------------------------------- dispatch --
// From run-time values to template arguments: with_*(value..., f) calls the generic lambda f with the value as a constant
// (decltype(X)::value inside f), once per value the kernels are compiled for. The order of the cases is the order in
// which the kernels are instantiated, which is their order in the code object.
template <int V> using int_c = std::integral_constant<int, V>;

template <class F>
auto with_bool(bool a, F &&f)
{
    return a ? f(std::true_type{}) : f(std::false_type{});
}

template <class F>
auto with_bools(bool a, bool b, F &&f)
{
    return with_bool(a, [&](auto A) { return with_bool(b, [&](auto B) { return f(A, B); }); });
}

// the beam kernels take a level's 4 x width children 64 per pass and are compiled for 1, 2, 4 and 8 passes
inline int passes_for_width(int width) { return width <= 16 ? 1 : width <= 32 ? 2 : width <= 64 ? 4 : 8; }

template <class F>
auto with_passes(int width, F &&f)
{
    switch (passes_for_width(width)) {
        case 1: return f(int_c<1>{});
        case 2: return f(int_c<2>{});
        case 4: return f(int_c<4>{});
        default: return f(int_c<8>{});
    }
}

}  // namespace g2048
