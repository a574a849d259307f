// g2048_per.hip -- the hybrid agent's prioritized experience replay on the device, for gfx950 (C-ABI: include/g2048.h).
//
//   PrioritizedReplayBuffer (agents/hybrid.py:730-765) as a ring in caller-owned arrays (layout and the push rule: g2048_per.h):
//     push     per_max_kernel (the maximum of the live priorities: an integer max on the bits of the positive floats), then
//              per_push_kernel (the scatter).
//     sample   w = p^alpha, probs = w / sum(w) in float32, the float64 cdf of np.random.choice, the search of the draws, the
//              importance weights, the gathered batch as DQNAgent.train_step builds it (:961-969) and its shaped rewards
//              (:971-1034). Seven stream-ordered launches: tile sums -> one wave over the sums -> the final pass, twice (sum(w),
//              then the cdf), the search, the weights' normalisation. No block waits for another one inside a launch, and no sum
//              goes through a floating-point atomic: every value is the same bits from run to run.
//     update   per_update_*: the occurrence latest in the batch wins a slot (an integer max of the batch position), then writes.
//   g2048_dqn_shape_rewards: the shaping alone, one lane per transition.
// Compile with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "../../include/g2048.h"
#include "g2048_board.h"
#include "g2048_host.h"
#include "g2048_per.h"
#include "g2048_per_max.h"
#include "g2048_rng.h"

using namespace g2048;

namespace {

constexpr int kPerTile = G2048_PER_SCAN_TILE;         // entries per block of the scan: one per thread
static_assert(kPerTile == kPerBlock, "the scan takes one entry per thread");
constexpr int kPerSearchBlock = 64;                   // samples per block of the search: a batch of 256 spreads over four CUs

// ---- workspace of a sample call -------------------------------------------------------------------------------------------
struct PerHeader {
    double total;            // the last entry of the un-normalised cdf
    float wsum;              // sum of p^alpha, rounded to float32
    uint32_t wmax_bits;      // the largest un-normalised weight of the batch
    uint32_t pad[12];
};
static_assert(sizeof(PerHeader) == 64, "the header keeps the arrays behind it aligned");

struct PerWorkspace {
    PerHeader *hdr;
    double *cdf;             // [size]
    double *tile_w;          // [tiles] sums of p^alpha
    double *tile_p;          // [tiles] sums of probs, then what lies before the tile
    float *probs;            // [size]
};

inline size_t per_tiles(size_t size) { return (size + kPerTile - 1) / kPerTile; }

inline size_t per_sample_workspace_bytes(size_t size)
{
    return sizeof(PerHeader) + (size + 2u * per_tiles(size)) * sizeof(double) + ((size + 3u) & ~(size_t)3u) * sizeof(float);
}

inline PerWorkspace per_workspace(void *base, size_t size)
{
    PerWorkspace w;
    w.hdr = static_cast<PerHeader *>(base);
    w.cdf = reinterpret_cast<double *>(w.hdr + 1);
    w.tile_w = w.cdf + size;
    w.tile_p = w.tile_w + per_tiles(size);
    w.probs = reinterpret_cast<float *>(w.tile_p + per_tiles(size));
    return w;
}

// ---- sums in a fixed order ------------------------------------------------------------------------------------------------
// the block's sum, in every thread: a butterfly inside the wave, the four waves in order
__device__ __forceinline__ double block_sum(double v, double *s_wave)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63u) == 0u) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    v = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
    __syncthreads();
    return v;
}

// inclusive running sum over the block's threads in thread order
__device__ __forceinline__ double block_scan(double v, double *s_wave)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_up(v, off);
        if (lane >= (uint32_t)off) v += o;
    }
    if (lane == 63u) s_wave[wave] = v;
    __syncthreads();
    double before = 0.0;
    for (uint32_t q = 0; q < wave; ++q) before += s_wave[q];
    __syncthreads();
    return wave ? before + v : v;
}

// ---- push -----------------------------------------------------------------------------------------------------------------
// (per_max_kernel, the maximum of the live priorities, and the two stream operations that run it: g2048_per_max.h)
template <bool REWARD_F64>
__global__ __launch_bounds__(kPerBlock) void per_push_kernel(uint4 *__restrict__ states, uint4 *__restrict__ next_states, uint8_t *__restrict__ actions,
                                                            float *__restrict__ rewards, uint8_t *__restrict__ dones, float *__restrict__ priorities,
                                                            size_t capacity, size_t size, size_t head, const uint4 *__restrict__ boards,
                                                            const uint4 *__restrict__ next_boards, const uint8_t *__restrict__ actions_in,
                                                            const void *__restrict__ rewards_in, const uint8_t *__restrict__ flags, size_t m,
                                                            const uint32_t *__restrict__ max_bits)
{
    const size_t k = (size_t)blockIdx.x * kPerBlock + threadIdx.x;
    if (k >= m) return;
    // entry k lands behind the size + k entries before it; the ring overwrites the oldest ones once it is full
    const size_t slot = (head + size + k) % capacity;
    states[slot] = boards[k];
    next_states[slot] = next_boards[k];
    actions[slot] = actions_in[k];
    rewards[slot] = REWARD_F64 ? (float)static_cast<const double *>(rewards_in)[k] : static_cast<const float *>(rewards_in)[k];
    dones[slot] = flags[k] & G2048_FLAG_DONE;
    priorities[slot] = size ? __uint_as_float(*max_bits) : 1.0f;
}

// ---- sample ---------------------------------------------------------------------------------------------------------------
// probs <- p^alpha (float32, un-normalised for now), tile_w <- the tile's sum of them
__global__ __launch_bounds__(kPerBlock) void per_weights_kernel(const float *__restrict__ priorities, size_t capacity, size_t size, size_t head,
                                                               float alpha, float *__restrict__ w_out, double *__restrict__ tile_w)
{
    __shared__ double s_wave[4];
    const size_t i = (size_t)blockIdx.x * kPerTile + threadIdx.x;
    float w = 0.0f;
    if (i < size) {
        w = powf(priorities[per_slot(head, i, capacity)], alpha);
        w_out[i] = w;
    }
    const double sum = block_sum((double)w, s_wave);
    if (threadIdx.x == 0) tile_w[blockIdx.x] = sum;
}

// one wave: wsum <- the sum of the tiles' sums, each lane its tiles in order, then the butterfly; the batch's weight maximum <- 0
__global__ __launch_bounds__(64) void per_wsum_kernel(const double *__restrict__ tile_w, size_t tiles, PerHeader *hdr)
{
    double v = 0.0;
    for (size_t t = threadIdx.x; t < tiles; t += 64u) v += tile_w[t];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (threadIdx.x == 0) {
        hdr->wsum = (float)v;
        hdr->wmax_bits = 0u;
    }
}

// the tile's probs and their running sum in float64, as both passes over the tiles compute it (the same bits in both)
__device__ __forceinline__ double per_tile_scan(const float *w, size_t size, float wsum, double *s_wave, float &prob)
{
    const size_t i = (size_t)blockIdx.x * kPerTile + threadIdx.x;
    prob = i < size ? w[i] / wsum : 0.0f;
    return block_scan((double)prob, s_wave);
}

// tile_p <- the running sum at the tile's last entry
__global__ __launch_bounds__(kPerBlock) void per_tile_sums_kernel(const float *__restrict__ w, size_t size, const PerHeader *__restrict__ hdr,
                                                                 double *__restrict__ tile_p)
{
    __shared__ double s_wave[4];
    float prob;
    const double run = per_tile_scan(w, size, hdr->wsum, s_wave, prob);
    const size_t last = min((size_t)blockIdx.x * kPerTile + (kPerTile - 1), size - 1u);
    if ((size_t)blockIdx.x * kPerTile + threadIdx.x == last) tile_p[blockIdx.x] = run;
}

// one wave: tile_p[t] <- the sum of the tiles before t, 64 tiles per round with the rounds' carry; total <- what lies before the
// last tile plus its sum, added exactly as the final pass adds them
__global__ __launch_bounds__(64) void per_scan_tiles_kernel(double *tile_p, size_t tiles, PerHeader *hdr)
{
    double carry = 0.0;
    for (size_t base = 0; base < tiles; base += 64u) {
        const size_t t = base + threadIdx.x;
        const double v = t < tiles ? tile_p[t] : 0.0;
        double inc = v;
        for (int off = 1; off < 64; off <<= 1) {
            const double o = __shfl_up(inc, off);
            if (threadIdx.x >= (uint32_t)off) inc += o;
        }
        const double up = __shfl_up(inc, 1);
        const double before = threadIdx.x ? carry + up : carry;
        if (t < tiles) tile_p[t] = before;
        if (t == tiles - 1u) hdr->total = before + v;
        carry += __shfl(inc, 63);
    }
}

// probs <- w / wsum, cdf <- (what lies before the tile + the running sum inside it) / total; the last entry is total / total
__global__ __launch_bounds__(kPerBlock) void per_cdf_kernel(float *__restrict__ w_probs, size_t size, const PerHeader *__restrict__ hdr,
                                                           const double *__restrict__ tile_before, double *__restrict__ cdf,
                                                           float *__restrict__ probs_out)
{
    __shared__ double s_wave[4];
    float prob;
    const double run = per_tile_scan(w_probs, size, hdr->wsum, s_wave, prob);
    const size_t i = (size_t)blockIdx.x * kPerTile + threadIdx.x;
    if (i >= size) return;
    cdf[i] = (tile_before[blockIdx.x] + run) / hdr->total;
    w_probs[i] = prob;
    if (probs_out) probs_out[i] = prob;
}

__device__ __forceinline__ float4 per_row_values(uint32_t x)
{
    return make_float4(per_tile_value(x & 0xffu), per_tile_value((x >> 8) & 0xffu), per_tile_value((x >> 16) & 0xffu), per_tile_value(x >> 24));
}

// sample j: its draw, the number of cdf entries <= the draw (searchsorted(side='right')), the transition there as train_step's
// tensors, its shaped reward and its un-normalised importance weight
__global__ __launch_bounds__(kPerSearchBlock) void per_search_kernel(
    const uint4 *__restrict__ states, const uint4 *__restrict__ next_states, const uint8_t *__restrict__ actions, const float *__restrict__ rewards,
    const uint8_t *__restrict__ dones, size_t capacity, size_t size, size_t head, float beta, size_t batch, uint32_t k0, uint32_t k1,
    const double *__restrict__ u_in, const double *__restrict__ cdf, const float *__restrict__ probs, PerHeader *hdr,
    long long *__restrict__ indices_out, float *__restrict__ weights_out, float4 *__restrict__ states_out, long long *__restrict__ actions_out,
    float *__restrict__ rewards_out, float4 *__restrict__ next_states_out, float *__restrict__ dones_out, float *__restrict__ shaped_out)
{
    const size_t j = (size_t)blockIdx.x * kPerSearchBlock + threadIdx.x;
    if (j >= batch) return;
    const double u = u_in ? u_in[j] : (double)rng_draw(k0, k1, (uint64_t)j, 0u) * 0x1p-32;
    size_t lo = 0, hi = size;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2u;
        if (cdf[mid] <= u) lo = mid + 1u;
        else hi = mid;
    }
    const size_t idx = lo < size ? lo : size - 1u;          // a draw of 1.0 or more has no entry above it: the last one
    const size_t slot = per_slot(head, idx, capacity);
    const uint4 sv = states[slot], nv = next_states[slot];
    const float reward = rewards[slot];
    indices_out[j] = (long long)idx;
    states_out[4u * j] = per_row_values(sv.x);
    states_out[4u * j + 1u] = per_row_values(sv.y);
    states_out[4u * j + 2u] = per_row_values(sv.z);
    states_out[4u * j + 3u] = per_row_values(sv.w);
    next_states_out[4u * j] = per_row_values(nv.x);
    next_states_out[4u * j + 1u] = per_row_values(nv.y);
    next_states_out[4u * j + 2u] = per_row_values(nv.z);
    next_states_out[4u * j + 3u] = per_row_values(nv.w);
    actions_out[j] = (long long)actions[slot];
    rewards_out[j] = reward;
    dones_out[j] = dones[slot] ? 1.0f : 0.0f;
    shaped_out[j] = dqn_shaped_reward(Board{{sv.x, sv.y, sv.z, sv.w}}, Board{{nv.x, nv.y, nv.z, nv.w}}, reward);
    const float w = powf((float)size * probs[idx], -beta);   // :754 float32 throughout
    weights_out[j] = w;
    atomicMax(&hdr->wmax_bits, __float_as_uint(w));          // positive floats: their bits order as they do
}

__global__ __launch_bounds__(kPerBlock) void per_normalise_kernel(float *__restrict__ weights, size_t batch, const PerHeader *__restrict__ hdr)
{
    const size_t j = (size_t)blockIdx.x * kPerBlock + threadIdx.x;
    if (j < batch) weights[j] = weights[j] / __uint_as_float(hdr->wmax_bits);
}

// ---- shaping alone --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPerBlock) void dqn_shape_kernel(const uint4 *__restrict__ states, const uint4 *__restrict__ next_states,
                                                             const float *__restrict__ rewards, size_t n, float *__restrict__ shaped)
{
    const size_t i = (size_t)blockIdx.x * kPerBlock + threadIdx.x;
    if (i >= n) return;
    const uint4 sv = states[i], nv = next_states[i];
    shaped[i] = dqn_shaped_reward(Board{{sv.x, sv.y, sv.z, sv.w}}, Board{{nv.x, nv.y, nv.z, nv.w}}, rewards[i]);
}

// ---- update_priorities ----------------------------------------------------------------------------------------------------
// Three passes over the batch, each its own launch: the touched slots' cells of the workspace to zero; every occurrence raises its
// slot's cell to its batch position + 1; the occurrence that finds its own position there -- the latest one -- writes.
__device__ __forceinline__ bool per_update_slot(const long long *indices, size_t batch, size_t capacity, size_t size, size_t head, size_t &j,
                                                size_t &slot)
{
    j = (size_t)blockIdx.x * kPerBlock + threadIdx.x;
    if (j >= batch) return false;
    const long long idx = indices[j];
    if (idx < 0 || (unsigned long long)idx >= size) return false;          // :761 beyond the live entries: ignored
    slot = per_slot(head, (size_t)idx, capacity);
    return true;
}

__global__ __launch_bounds__(kPerBlock) void per_update_clear_kernel(const long long *__restrict__ indices, size_t batch, size_t capacity, size_t size,
                                                                    size_t head, uint32_t *__restrict__ winner)
{
    size_t j, slot;
    if (per_update_slot(indices, batch, capacity, size, head, j, slot)) winner[slot] = 0u;
}

__global__ __launch_bounds__(kPerBlock) void per_update_claim_kernel(const long long *__restrict__ indices, size_t batch, size_t capacity, size_t size,
                                                                    size_t head, uint32_t *winner)
{
    size_t j, slot;
    if (per_update_slot(indices, batch, capacity, size, head, j, slot)) atomicMax(&winner[slot], (uint32_t)j + 1u);
}

__global__ __launch_bounds__(kPerBlock) void per_update_write_kernel(const long long *__restrict__ indices, const float *__restrict__ td_errors,
                                                                    size_t batch, size_t capacity, size_t size, size_t head,
                                                                    const uint32_t *__restrict__ winner, float *__restrict__ priorities)
{
    size_t j, slot;
    if (per_update_slot(indices, batch, capacity, size, head, j, slot) && winner[slot] == (uint32_t)j + 1u)
        priorities[slot] = per_priority(td_errors[j]);
}

constexpr size_t kPerMaxBatch = (size_t)1 << 31;      // batch positions are 32-bit in the update's workspace

}  // namespace

// ==================================================================== C-ABI ====
extern "C" {

size_t g2048_per_update_workspace(size_t capacity) { return (capacity ? capacity : 1u) * sizeof(uint32_t); }

int g2048_per_push(void *states, void *next_states, uint8_t *actions, float *rewards, uint8_t *dones, float *priorities, size_t capacity,
                   size_t size, size_t head, const void *boards, const void *next_boards, const uint8_t *actions_in, const void *rewards_in,
                   uint32_t rewards_f64, const uint8_t *flags, size_t m, void *workspace, void *stream)
{
    if (m > capacity) return fail(G2048_ERR_ARG, "g2048_per_push: more transitions than the buffer's capacity (m = %zu, capacity %zu)", m, capacity);
    if (m == 0) return G2048_OK;
    if (!states || !next_states || !actions || !rewards || !dones || !priorities || !boards || !next_boards || !actions_in || !rewards_in ||
        !flags || !workspace)
        return fail(G2048_ERR_ARG, "g2048_per_push: null pointer");
    if (size > capacity || head >= capacity) return fail(G2048_ERR_ARG, "g2048_per_push: size must be at most capacity and head below it");
    if (!aligned(states, 16) || !aligned(next_states, 16) || !aligned(boards, 16) || !aligned(next_boards, 16) || !aligned(rewards, 4) ||
        !aligned(priorities, 4) || !aligned(rewards_in, rewards_f64 ? 8 : 4) || !aligned(workspace, 4))
        return fail(G2048_ERR_ARG, "g2048_per_push: misaligned array (boards: 16 bytes)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint32_t *max_bits = static_cast<uint32_t *>(workspace);
    if (size) {
        const int rc = per_max_enqueue("g2048_per_push: hipMemsetAsync", priorities, capacity, size, head, max_bits, s);
        if (rc != G2048_OK) return rc;
    }
    with_bool(rewards_f64 != 0u, [&](auto F) {
        hipLaunchKernelGGL((per_push_kernel<decltype(F)::value>), dim3(blocks_for(m, kPerBlock)), dim3(kPerBlock), 0, s, static_cast<uint4 *>(states),
                           static_cast<uint4 *>(next_states), actions, rewards, dones, priorities, capacity, size, head,
                           static_cast<const uint4 *>(boards), static_cast<const uint4 *>(next_boards), actions_in, rewards_in, flags, m, max_bits);
    });
    return check_launch("g2048_per_push");
}

size_t g2048_per_sample_workspace(size_t size, size_t batch)
{
    (void)batch;
    return per_sample_workspace_bytes(size ? size : 1u);
}

int g2048_per_sample(const void *states, const void *next_states, const uint8_t *actions, const float *rewards, const uint8_t *dones,
                     const float *priorities, size_t capacity, size_t size, size_t head, float alpha, float beta, size_t batch, uint64_t seed,
                     uint64_t sample_index, const double *u_or_null, void *workspace, int64_t *indices_out, float *weights_out,
                     float *states_out, int64_t *actions_out, float *rewards_out, float *next_states_out, float *dones_out, float *shaped_out,
                     float *probs_out_or_null, void *stream)
{
    if (size < batch)
        return fail(G2048_ERR_ARG, "g2048_per_sample: fewer live entries than the batch (size %zu, batch %zu): train_step does not sample then", size,
                    batch);
    if (batch == 0) return G2048_OK;
    if (!states || !next_states || !actions || !rewards || !dones || !priorities || !workspace || !indices_out || !weights_out || !states_out ||
        !actions_out || !rewards_out || !next_states_out || !dones_out || !shaped_out)
        return fail(G2048_ERR_ARG, "g2048_per_sample: null pointer");
    if (size > capacity || head >= capacity) return fail(G2048_ERR_ARG, "g2048_per_sample: size must be at most capacity and head below it");
    if (batch > kPerMaxBatch || per_tiles(size) > 0x7fffffffu) return fail(G2048_ERR_ARG, "g2048_per_sample: too large for one call");
    if (!aligned(states, 16) || !aligned(next_states, 16) || !aligned(states_out, 16) || !aligned(next_states_out, 16) || !aligned(workspace, 16) ||
        !aligned(u_or_null, 8) || !aligned(indices_out, 8) || !aligned(actions_out, 8) || !aligned(rewards, 4) || !aligned(priorities, 4) ||
        !aligned(weights_out, 4) || !aligned(rewards_out, 4) || !aligned(dones_out, 4) || !aligned(shaped_out, 4) || !aligned(probs_out_or_null, 4))
        return fail(G2048_ERR_ARG, "g2048_per_sample: misaligned array (boards, states and the workspace: 16 bytes)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const PerWorkspace w = per_workspace(workspace, size);
    const unsigned tiles = (unsigned)per_tiles(size);
    const Keys k = rng_keys(seed, DOM_REPLAY, sample_index);
    hipLaunchKernelGGL(per_weights_kernel, dim3(tiles), dim3(kPerBlock), 0, s, priorities, capacity, size, head, alpha, w.probs, w.tile_w);
    hipLaunchKernelGGL(per_wsum_kernel, dim3(1), dim3(64), 0, s, w.tile_w, (size_t)tiles, w.hdr);
    hipLaunchKernelGGL(per_tile_sums_kernel, dim3(tiles), dim3(kPerBlock), 0, s, w.probs, size, w.hdr, w.tile_p);
    hipLaunchKernelGGL(per_scan_tiles_kernel, dim3(1), dim3(64), 0, s, w.tile_p, (size_t)tiles, w.hdr);
    hipLaunchKernelGGL(per_cdf_kernel, dim3(tiles), dim3(kPerBlock), 0, s, w.probs, size, w.hdr, w.tile_p, w.cdf, probs_out_or_null);
    hipLaunchKernelGGL(per_search_kernel, dim3(blocks_for(batch, kPerSearchBlock)), dim3(kPerSearchBlock), 0, s, static_cast<const uint4 *>(states),
                       static_cast<const uint4 *>(next_states), actions, rewards, dones, capacity, size, head, beta, batch, k.k0, k.k1, u_or_null,
                       w.cdf, w.probs, w.hdr, reinterpret_cast<long long *>(indices_out), weights_out, reinterpret_cast<float4 *>(states_out),
                       reinterpret_cast<long long *>(actions_out), rewards_out, reinterpret_cast<float4 *>(next_states_out), dones_out, shaped_out);
    hipLaunchKernelGGL(per_normalise_kernel, dim3(blocks_for(batch, kPerBlock)), dim3(kPerBlock), 0, s, weights_out, batch, w.hdr);
    return check_launch("g2048_per_sample");
}

int g2048_dqn_shape_rewards(const void *states, const void *next_states, const float *rewards, size_t n, float *shaped_out, void *stream)
{
    if (n == 0) return G2048_OK;
    if (!states || !next_states || !rewards || !shaped_out) return fail(G2048_ERR_ARG, "g2048_dqn_shape_rewards: null pointer");
    if (!aligned(states, 16) || !aligned(next_states, 16) || !aligned(rewards, 4) || !aligned(shaped_out, 4))
        return fail(G2048_ERR_ARG, "g2048_dqn_shape_rewards: misaligned array (boards: 16 bytes)");
    if (blocks_for(n, kPerBlock) > 0x7fffffffu) return fail(G2048_ERR_ARG, "g2048_dqn_shape_rewards: too many transitions for one call");
    hipLaunchKernelGGL(dqn_shape_kernel, dim3(blocks_for(n, kPerBlock)), dim3(kPerBlock), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint4 *>(states), static_cast<const uint4 *>(next_states), rewards, n, shaped_out);
    return check_launch("g2048_dqn_shape_rewards");
}

int g2048_per_update_priorities(float *priorities, size_t capacity, size_t size, size_t head, const int64_t *indices, const float *td_errors,
                                size_t batch, void *workspace, void *stream)
{
    if (batch == 0) return G2048_OK;
    if (!priorities || !indices || !td_errors || !workspace) return fail(G2048_ERR_ARG, "g2048_per_update_priorities: null pointer");
    if (size > capacity || (capacity && head >= capacity))
        return fail(G2048_ERR_ARG, "g2048_per_update_priorities: size must be at most capacity and head below it");
    if (batch > kPerMaxBatch) return fail(G2048_ERR_ARG, "g2048_per_update_priorities: batch too large for one call");
    if (!aligned(priorities, 4) || !aligned(indices, 8) || !aligned(td_errors, 4) || !aligned(workspace, 4))
        return fail(G2048_ERR_ARG, "g2048_per_update_priorities: misaligned array");
    if (size == 0) return G2048_OK;                   // every index is beyond the live entries
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid(blocks_for(batch, kPerBlock)), block(kPerBlock);
    const long long *idx = reinterpret_cast<const long long *>(indices);
    uint32_t *winner = static_cast<uint32_t *>(workspace);
    hipLaunchKernelGGL(per_update_clear_kernel, grid, block, 0, s, idx, batch, capacity, size, head, winner);
    hipLaunchKernelGGL(per_update_claim_kernel, grid, block, 0, s, idx, batch, capacity, size, head, winner);
    hipLaunchKernelGGL(per_update_write_kernel, grid, block, 0, s, idx, td_errors, batch, capacity, size, head, winner, priorities);
    return check_launch("g2048_per_update_priorities");
}

}  // extern "C"
