// bdrt_nuts_launch.h -- what the sampler driver (bdrt_sampler.hip) needs from the translation units that hold the sampler kernels:
// the LDS sizes of the one-chain kernels, and one launch_* function per kernel family (bdrt_nuts.hip: 16-chain, one-chain-per-
// workgroup, streamed, re-layout kernels; bdrt_wave.hip: one chain per wave).  A launch_* function returns 0 or, after set_error, < 0.
#pragma once
#include "bdrt_nuts16.h"

namespace bdrt {

// ---- nuts_wide1_kernel: the evaluator's LDS, the cooperative stage's scratch (reductions, momentum normals), `nhot` rows of the chain
constexpr int W1_SCRATCH = 1600;
constexpr int W1_HOT_MAX = 12;
__host__ __device__ inline size_t wide1_lds_bytes(const Wide1Geom &G, int ds, int nhot)
{
    return ((size_t)G.total + W1_SCRATCH + 2 + (size_t)nhot * ds) * sizeof(double) + sizeof(ChainState) + 64 + 64;
}
static_assert((W1_SCRATCH + 2) * sizeof(double) + sizeof(ChainState) + 128 <= 16384, "wide1_capable (bdrt_solo_wide.h) leaves 16 KiB beside the evaluator");

// ---- nuts_big_kernel<NJX>: D <= 512 NJX
constexpr int BIG_MAX_D = 8192;
__host__ __device__ inline int big_njx(int D) { return D <= 1024 ? 2 : (D <= 2048 ? 4 : (D <= 4096 ? 8 : 16)); }
__host__ __device__ inline int big_scratch_doubles(int njx) { return njx <= 2 ? W1_SCRATCH : 512 + 512 * njx + 64; }
__host__ __device__ inline size_t nuts_big_lds_bytes(int njx = 2) { return (size_t)(big_scratch_doubles(njx) + 2 + 9 * 8) * sizeof(double) + sizeof(ChainState) + 128; }

// ---- nuts_solo_kernel with two workgroups per CU: SOLO_NHOT rows of the chain in LDS (one per CU: all rows, SoloGeom::total doubles + 64)
inline size_t solo_duo_lds_bytes(const SoloGeom &g) { return ((size_t)g.o_vec + (size_t)SOLO_NHOT * g.DSS) * sizeof(double) + 64; }

// A sampler instantiation by its key.  tile16: nuts_kernel<a, b, c> = <NJ, MODE, TA (MODE 2) or KU (MODES 3, 4)>, one of
// BDRT_NUTS16_G0..G5; solo: nuts_solo_kernel<a> (a = 2: one workgroup per CU, 4: two); wide1: nuts_wide1_kernel; big: nuts_big_kernel<a>
enum class NutsFamily { tile16, solo, wide1, big };
struct NutsKey {
    NutsFamily family;
    int a, b, c;
};
// every launch below needs at most `bytes` of dynamic LDS (hipFuncSetAttribute of all instantiations, per device, high-water mark)
hipError_t nuts_set_lds_limit(size_t bytes);
// The kernel of `key` -- its profiling instantiation when args.prof is set and there is one -- on (dp, np, args) and the kernel's
// further parameters (solo: extra0 = const SoloGeom *; wide1: const Wide1Geom *, extra1 = const int *nhot).  No such key: an error.
int launch_nuts(NutsKey key, const DevProblem *dp, const NutsParams &np, const NutsArgs &args, int n_wg, size_t lds, hipStream_t stream,
                const void *extra0 = nullptr, const void *extra1 = nullptr);
// re-layout between launches: live[u] = chain u is still running; the live chains' 16-chain rows -> one-chain rows (to_solo: those of
// nuts_solo_kernel, stride dss; else one column, same stride); 16-chain rows -> fewer 16-chain workgroups
int launch_nuts_live(const ChainState *states, int n_units, int *live, hipStream_t stream);
int launch_nuts_migrate(bool to_solo, const double *v16, int ds16, const int *unit_loc, const int *unit_map, int n_tail, double *vnew, int dss,
                        int D, ChainState *states, hipStream_t stream);
int launch_nuts_compact(const double *vold, const int *old_loc, const int *new_slot_unit, int n_wg, double *vnew, int ds, hipStream_t stream);

// one-chain-per-wave sampler / evaluator (bdrt_wave.hip)
size_t wave_lds_request(const WaveGeom &g, int n_wg, int n_cu, int *nhot, int max_per_cu);
int launch_wave_nuts(const DevProblem *dp, const NutsParams &np, const NutsArgs &args, const WaveGeom &g, int nhot, int n_wg, size_t lds,
                     hipStream_t stream, int outlier_model);
int launch_wave_eval(const DevProblem *dp, const WaveGeom &g, const double *d_theta, const int *d_spec, int B, int jacobian, double *d_lp,
                     double *d_grad, int n_wg, size_t lds, hipStream_t stream, int outlier_model);

}  // namespace bdrt
