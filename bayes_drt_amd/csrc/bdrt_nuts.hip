// bdrt_nuts.hip -- device-resident NUTS (replaces StanModel.sampling, reference bayes_drt/inversion.py:1218-1221): the one-chain-per-
// workgroup, streamed and re-layout kernels, the launchers of these and of the 16-chain kernel (bdrt_nuts_launch.h), and the few-point
// evaluator / device L-BFGS that launch kernels of this file.  The sampler's host side is bdrt_sampler.hip.
//
// MI355X design: one workgroup owns 16 chains for the whole run.  Every loop iteration is one leapfrog for those
// 16 chains: kick/drift (vector pass), the MFMA log-posterior+gradient tile (bdrt_device.h), second kick, then the
// NUTS bookkeeping (multinomial sampling, U-turn checks, tree doubling, step-size / metric adaptation) -- all on
// the device, so there is no host round trip per gradient evaluation.  Chains are asynchronous: each advances
// through its own iterations / tree depths; only the leapfrog itself is lock-step inside a workgroup.  The host
// relaunches the kernel in bounded slices (`rounds` leapfrogs per launch) and never reads anything back until
// the end; workgroups never communicate, so there is no grid barrier and no inter-workgroup hand-off.
//
// Algorithm: Stan 2.19 multinomial NUTS with diagonal metric:
//   * tree doubling with uniform direction, biased progressive sampling between the old trajectory and the new
//     subtree, uniform (multinomial) sampling inside the new subtree -- realised as weighted reservoir sampling
//     over the leaves in generation order (same distribution as Stan's pairwise merging);
//   * generalised U-turn criterion p#_left.rho > 0 && p#_right.rho > 0 on every completed sub-subtree; the
//     sub-subtree rho's are kept per level (binary counter over the leaf index), summed in the order of the recursion;
//   * divergence when H - H0 > 1000; max tree depth 10;
//   * warm-up: step-size heuristic + dual averaging (delta, gamma, t0, kappa), windowed diagonal metric
//     (init_buffer 75 / base_window 25 doubling / term_buffer 50, regularised variance).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "bdrt_nuts_launch.h"

namespace bdrt {
// (defined in bdrt_nuts_k0.hip .. bdrt_nuts_k5.hip)
BDRT_NUTS16_G0(BDRT_NUTS16_DECLARE) BDRT_NUTS16_G1(BDRT_NUTS16_DECLARE) BDRT_NUTS16_G2(BDRT_NUTS16_DECLARE)
BDRT_NUTS16_G3(BDRT_NUTS16_DECLARE) BDRT_NUTS16_G4(BDRT_NUTS16_DECLARE) BDRT_NUTS16_G5(BDRT_NUTS16_DECLARE_PROF)

// ---------------------------------------------------------------------------------------------------------------------------
// One chain per workgroup (bdrt_solo.h): the same transition logic as nuts_kernel, element j of every vector in thread j,
// all vectors in LDS.  Global state layout: vecs [n_units][SG_COUNT][ds]; states [n_units].
// ---------------------------------------------------------------------------------------------------------------------------

template <int WPE, bool PROF = false>   // waves per SIMD the register budget allows: 2 = one workgroup per CU, 4 = two (when their LDS fits); PROF: fills the phase profile
__global__ __launch_bounds__(SOLO_NT, WPE) void nuts_solo_kernel(const DevProblem *__restrict__ Pp, NutsParams np, NutsArgs a, SoloGeom g)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const DevProblem &P = *Pp;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int unit = a.unit_map ? a.unit_map[blockIdx.x] : blockIdx.x;
    const int D = g.D, DS = a.ds, j = tid;
    const bool own = j < D;                                // this thread owns element j of the D-vectors
    double *Vg = a.vecs + (size_t)blockIdx.x * SG_COUNT * DS;    // global rows
    double *V = smem + g.o_vec;                            // LDS rows
    // WPE 4 (two workgroups per CU): SOLO_NHOT rows in LDS, the others where they are in HBM (each thread touches its own element)
    constexpr bool TRIM = WPE == 4;
    auto row = [&](int v) -> double * {
        if constexpr (!TRIM) return V + (size_t)v * g.DSS;
        else { const int h = solo_hot_slot(v); return h >= 0 ? V + (size_t)h * g.DSS : Vg + (size_t)v * DS; }
    };
    double *red = smem + g.o_red;
    double *zrow = smem + g.o_z;
    double *lps_l = smem + g.o_scv + 12;                   // lp of the last evaluation
    int slot = 0;

    // the chain's scalar state lives in LDS; every thread keeps its hot part in registers (identical updates)
    ChainState *cold = reinterpret_cast<ChainState *>(smem + g.o_state);
    if (tid == 0) chain_state_copy(*cold, a.states[unit]);          // (member by member: a struct assignment goes through scratch)
#pragma unroll 7
    for (int v = 0; v < SV_COUNT; ++v) {
        if (TRIM && solo_hot_slot(v) < 0) continue;
        const double x = own ? Vg[(size_t)v * DS + j] : 0.0;
        if (j < g.DSS) row(v)[j] = x;
    }
    solo_eval_init(P, g, smem, tid);
    __syncthreads();
    // one workgroup per CU: the whole state in registers (256 VGPRs to spend); two per CU: the hot part only
    typedef typename std::conditional<WPE == 2, ChainState, SoloHot>::type State;
    State s;
    if constexpr (WPE == 2) chain_state_copy(s, *cold); else s.from(*cold);
    const Philox rng = {np.seed_lo, np.seed_hi, (uint32_t)cold->chain_id};
    const SoloEvalRegs er = solo_eval_setup(P, g, cold->spec, tid);
    double *TH = row(SV_TH), *Pm = row(SV_P), *G = row(SV_G), *MI = row(SV_MINV);
    // a statement of the shared scalar logic that needs the whole state: assembled from LDS + registers, run identically by
    // every thread, written back by one (all threads take this path together: the state is uniform)
    auto with_full_state = [&](auto fn) {
        if constexpr (WPE == 2) return fn(s);
        else {
            ChainState full;
            chain_state_copy(full, *cold);
            s.to(full);
            const int r = fn(full);
            s.from(full);
            __syncthreads();
            if (tid == 0) chain_state_copy(*cold, full);
            __syncthreads();
            return r;
        }
    };

    if (!cold->kicked) {
        const int ph = s.phase;
        const double e = ph == PH_EPS ? s.eps : (ph == PH_TREE ? s.dir * s.eps : 0.0);
        if ((ph == PH_INIT || ph == PH_EPS || ph == PH_TREE) && own) {
            const double p = Pm[j] + 0.5 * e * G[j];
            Pm[j] = p;
            TH[j] += e * MI[j] * p;
        }
        __syncthreads();
        if (tid == 0) cold->kicked = 1;
        __syncthreads();
    }
    unsigned long long my_leaps = 0;

    for (int round = 0; round < a.rounds; ++round) {
        const int ph0 = s.phase;
        const bool act = ph0 == PH_INIT || ph0 == PH_EPS || ph0 == PH_TREE;
        if (!act) break;
        const double e = ph0 == PH_EPS ? s.eps : (ph0 == PH_TREE ? s.dir * s.eps : 0.0);

        // ---- B: log-posterior + gradient at the new point ------------------------------------------------------------------
        long long *prof = (PROF && a.prof) ? a.prof + (size_t)unit * 32 : nullptr;
        // the uniform that decides whether this leaf replaces the subtree's proposal depends on (leaf, depth, iteration)
        // only: wave 7, which has no per-element work in the first phases of the evaluation, draws it now (Philox, ~200
        // integer instructions) and publishes it through LDS, off the other waves' critical path
        if (ph0 == PH_TREE && wave == SOLO_NW - 1) {
            const double u = rng_uniform(rng, (uint32_t)s.leaf, RNG_LEAF, (uint32_t)s.depth, 0, (uint32_t)s.iter);
            if (lane == 0) lps_l[1] = u;
        }
        solo_eval<WPE == 2 ? 16 : 8>(P, g, smem, TH, G, lps_l, er, 1, tid, prof);
        long long tsp = (prof && tid == 0) ? clock64() : 0;
#define BDRT_SOLO_NPROF(slot) do { if (prof && tid == 0) { const long long t_ = clock64(); prof[slot] += t_ - tsp; tsp = t_; } } while (0)

        // ---- C: second half kick, kinetic energy, finiteness of the gradient ----------------------------------------------------
        double p = 0.0, gj = 0.0, mi = 1.0;
        double kin = 0.0, nonfin = 0.0;
        if (own) {
            gj = G[j]; mi = MI[j];
            p = Pm[j] + 0.5 * e * gj;
            kin = mi * p * p;
            nonfin = isfinite(gj) ? 0.0 : 1.0;
        }
        // (measured and dropped: the U-turn products of the first three merge levels -- known from the leaf index -- in this same
        // block reduction: stages C + D 3.2 k -> 2.9 k cycles, the evaluation + 0.5 k from the registers it takes; 6.12 -> 6.32 us)
        solo_block_sum2(kin, nonfin, red, slot, wave, lane);
        kin *= 0.5;
        BDRT_SOLO_NPROF(5);

        // ---- S1: scalar logic after the evaluation (identical in every thread) ---------------------------------------------------
        bool copyq = false, cur2s = false, tree = false, last = false;
        bool upds = false, welf = false, wend = false;
        int nm = 0, endt = 0, next = 0, draw = -1;
        double wn = 0.0;
        const int dir_now = s.dir;
        const int leaf_now = s.leaf;
        {
            const double lp = *lps_l;
            const bool finite_pt = isfinite(lp) && nonfin == 0.0;
            if (ph0 == PH_INIT) {
                if (finite_pt) {
                    s.lps = lp;
                    cur2s = true;
                    s.phase = PH_EPS; s.eps_dir = 0; s.eps_trials = 0;
                    next = 3;
                } else {
                    const int att = s.init_attempt + 1;
                    s.init_attempt = att;
                    if (att >= 100) s.phase = PH_FAILED;
                    else next = 4;
                }
            } else if (ph0 == PH_EPS) {
                // Stan base_hmc::init_stepsize
                my_leaps += 1;
                next = with_full_state([&](ChainState &f) { return nuts_stepsize_trial(f, np, lp, kin); });
            } else {   // PH_TREE: one new leaf
                my_leaps += 1;
                s.n_leap_iter = s.n_leap_iter + 1;
                double h = -lp + kin;
                if (isnan(h)) h = INFINITY;
                const double H0 = s.H0;
                const bool divergent = (h - H0) > np.max_deltaH;
                const double w = H0 - h;
                s.sum_metro = s.sum_metro + (w > 0.0 ? 1.0 : BDRT_NUTS_EXP(fmax(w, -746.0)));       // (w = -inf on a non-finite energy)
                if (divergent) {
                    endt = 2;
                } else {
                    const double u = lps_l[1];                          // drawn by wave 7 before the evaluation
                    double lsw_new;
                    const bool joins = nuts_leaf_joins(s.lsw_sub, w, u, lsw_new);           // (one exponential: bdrt_nuts_device.h)
                    if (leaf_now == 0 || joins) { copyq = true; s.lpq = lp; }
                    s.lsw_sub = lsw_new;
                    tree = true;
                    while ((leaf_now >> nm) & 1) ++nm;
                    last = leaf_now == s.nleaves - 1;
                }
            }
        }

        BDRT_SOLO_NPROF(6);
        // ---- D: proposal copy, checkpoints, U-turn tests, subtree close ----------------------------------------------------------
        if ((copyq || cur2s) && own) {
            const double th = TH[j];
            if (copyq) { row(SV_THQ)[j] = th; row(SV_GQ)[j] = gj; }
            if (cur2s) { row(SV_THS)[j] = th; row(SV_GS)[j] = gj; }
        }
        if (tree) {
            // binary-counter bookkeeping of the new subtree: see nuts_kernel (level l: rho / first momentum of the completed
            // left sub-subtree of 2^l leaves that waits for its sibling; level 0 keeps only the momentum)
            double rc = p, cpl = p;
            bool ok = true;
            for (int l = 0; l < nm; ++l) {
                double a0 = 0.0, a1 = 0.0;
                if (own) {
                    const double lpv = row(SV_CKP + l)[j];
                    const double lr = l == 0 ? lpv : row(SV_CKC + l)[j];
                    const double rho = lr + rc;
                    a0 = mi * lpv * rho;
                    a1 = mi * p * rho;
                    rc = rho;
                    cpl = lpv;
                }
                solo_block_sum2(a0, a1, red, slot, wave, lane);
                ok = ok && (a0 > 0.0) && (a1 > 0.0);
            }
            if (ok && !last && own) {
                row(SV_CKP + nm)[j] = cpl;
                if (nm > 0) row(SV_CKC + nm)[j] = rc;
            }
            if (!ok) {
                endt = 1;
            } else if (last) {
                double t0 = 0.0, t1 = 0.0;
                if (own) {
                    const double po = row(dir_now > 0 ? SV_PM : SV_PP)[j];     // momentum at the other end
                    const double rt = row(SV_RHO)[j] + rc;
                    row(SV_RHO)[j] = rt;
                    row(dir_now > 0 ? SV_THP : SV_THM)[j] = TH[j];
                    row(dir_now > 0 ? SV_PP : SV_PM)[j] = p;
                    row(dir_now > 0 ? SV_GP : SV_GM)[j] = gj;
                    t0 = mi * po * rt;
                    t1 = mi * p * rt;
                }
                solo_block_sum2(t0, t1, red, slot, wave, lane);
                const int depth = s.depth + 1;
                s.depth = depth;
                const double lsw = s.lsw, lsw_sub = s.lsw_sub;
                bool take;
                if (lsw_sub > lsw) take = true;
                else take = rng_uniform(rng, 0, RNG_TOP, (uint32_t)depth, 0, (uint32_t)s.iter) < BDRT_NUTS_EXP(lsw_sub - lsw);
                if (take) { upds = true; s.lps = s.lpq; }
                s.lsw = log_sum_exp2(lsw, lsw_sub);
                const bool keep_going = (t0 > 0.0) && (t1 > 0.0);
                if (!keep_going || depth >= np.max_depth) endt = 1;
                else {
                    s.dir = rng_uniform(rng, 0, RNG_DIRECTION, (uint32_t)depth, 0, (uint32_t)s.iter) > 0.5 ? 1 : -1;
                    s.leaf = 0; s.nleaves = 1 << depth; s.lsw_sub = -INFINITY;
                    next = 2;
                }
            } else {
                s.leaf = leaf_now + 1;
            }
        }
        if (endt) {
            next = with_full_state([&](ChainState &f) { return nuts_transition_end(f, np, endt, draw, welf, wend, wn); });     // (bdrt_nuts_device.h)
            if (draw >= 0 && a.lp_draws && tid == 0) a.lp_draws[(size_t)unit * np.n_draws + draw] = s.lps;
        }

        BDRT_SOLO_NPROF(7);
        // ---- A': the trajectory continues from the point just evaluated: half kick + drift of the next leapfrog ---------------------
        if (next == 0 && s.phase == PH_TREE) {
            const double e1 = s.dir * s.eps;
            if (own) {
                const double pk = p + 0.5 * e1 * gj;
                Pm[j] = pk;
                TH[j] = TH[j] + e1 * mi * pk;
            }
        }
        // ---- E: sample update, metric adaptation, draw output, start of the next leapfrog when the trajectory does not simply
        //      continue (new transition, next doubling, step-size search, re-initialisation) ------------------------------------------
        if (upds || welf || wend || draw >= 0 || next) {
            const uint32_t iter = (uint32_t)s.iter, trial = (uint32_t)s.eps_trials, att = (uint32_t)s.init_attempt;
            double ths = 0.0, gs = 0.0;
            if (own && (upds || welf || wend || draw >= 0 || next == 1 || next == 3)) {
                ths = row(upds ? SV_THQ : SV_THS)[j]; gs = row(upds ? SV_GQ : SV_GS)[j];
            }
            if (upds && own) { row(SV_THS)[j] = ths; row(SV_GS)[j] = gs; }
            if ((welf || wend) && own) {
                double *WM = Vg + (size_t)SG_WMEAN * DS, *W2 = Vg + (size_t)SG_WM2 * DS;
                double mean = WM[j], m2 = W2[j];
                if (welf) {            // Welford (stan::math::welford_var_estimator)
                    const double delta = ths - mean;
                    mean += delta / wn;
                    m2 += (ths - mean) * delta;
                }
                if (wend) {            // var_adaptation::learn_variance
                    const double var = wn > 1.0 ? m2 / (wn - 1.0) : 0.0;
                    mi = (wn / (wn + 5.0)) * var + 1e-3 * (5.0 / (wn + 5.0));
                    MI[j] = mi;
                    mean = 0.0; m2 = 0.0;
                }
                WM[j] = mean; W2[j] = m2;
            }
            if (draw >= 0 && own) a.draws[((size_t)unit * np.n_draws + draw) * D + j] = ths;
            if (next == 1 || next == 3) {
                // fresh momentum p ~ N(0, M): normals 2i, 2i+1 from one Philox block (same streams as nuts_kernel)
                if (2 * tid < D) {
                    double z0, z1;
                    rng_normal_pair(rng, (uint32_t)tid, next == 1 ? RNG_MOMENTUM : RNG_EPS_MOMENTUM, next == 1 ? 0u : trial, iter, z0, z1);
                    zrow[2 * tid] = z0; zrow[2 * tid + 1] = z1;
                }
                __syncthreads();
                double pn = 0.0, kin0 = 0.0, dummy = 0.0;
                if (own) { pn = zrow[j] / sqrt(mi); kin0 = mi * pn * pn; }
                solo_block_sum2(kin0, dummy, red, slot, wave, lane);
                s.H0 = -s.lps + 0.5 * kin0;
                if (next == 1) {
                    s.lsw = 0.0; s.lsw_sub = -INFINITY; s.depth = 0; s.leaf = 0; s.nleaves = 1;
                    s.n_leap_iter = 0; s.sum_metro = 0.0;
                    s.dir = rng_uniform(rng, 0, RNG_DIRECTION, 0, 0, (uint32_t)s.iter) > 0.5 ? 1 : -1;
                }
                const double e1 = next == 1 ? s.dir * s.eps : s.eps;
                if (own) {
                    if (next == 1) {
                        row(SV_THM)[j] = ths; row(SV_THP)[j] = ths;
                        row(SV_PM)[j] = pn; row(SV_PP)[j] = pn;
                        row(SV_GM)[j] = gs; row(SV_GP)[j] = gs;
                        row(SV_RHO)[j] = pn;
                    }
                    const double pk = pn + 0.5 * e1 * gs;
                    Pm[j] = pk;
                    TH[j] = ths + e1 * mi * pk;
                }
            } else if (next == 2) {
                // continue from the trajectory end in the new direction
                const int dir = s.dir;
                const double e1 = dir * s.eps;
                if (own) {
                    double et, ep, eg;
                    if (dir == dir_now) { et = TH[j]; ep = p; eg = gj; }
                    else { et = row(dir > 0 ? SV_THP : SV_THM)[j]; ep = row(dir > 0 ? SV_PP : SV_PM)[j]; eg = row(dir > 0 ? SV_GP : SV_GM)[j]; }
                    const double pk = ep + 0.5 * e1 * eg;
                    Pm[j] = pk;
                    TH[j] = et + e1 * mi * pk;
                }
            } else if (next == 4) {
                if (own) {
                    TH[j] = np.init_radius * (2.0 * rng_uniform(rng, (uint32_t)j, RNG_INIT, 0, att, 0) - 1.0);
                    Pm[j] = 0.0;
                }
            }
        }
        __syncthreads();                                   // theta / momentum rows complete before the next evaluation
        BDRT_SOLO_NPROF(8);
#undef BDRT_SOLO_NPROF
    }

    // ---- write the chain back ---------------------------------------------------------------------------------------------------
    __syncthreads();
    for (int v = 0; v < SV_COUNT; ++v)
        if (own && !(TRIM && solo_hot_slot(v) < 0)) Vg[(size_t)v * DS + j] = row(v)[j];
    if (tid == 0) {
        ChainState full;
        chain_state_copy(full, *cold);
        if constexpr (WPE == 2) { const int k = full.kicked; full = s; full.kicked = k; } else s.to(full);
        chain_state_copy(a.states[unit], full);
        if (my_leaps) atomicAdd(a.leap_counter, my_leaps);
        const int ph = s.phase;
        if (!(ph == PH_INIT || ph == PH_EPS || ph == PH_TREE)) atomicAdd(a.done_counter, 1);
    }
}

// evaluator of the solo path on its own (few-point batches of bdrt_logp_grad, parity tests): a workgroup per point -- or, with
// fewer workgroups than points, a grid-stride loop over the points --, theta / grad [B x D] in global memory.  Needs only the
// evaluator's share of the LDS (solo_eval_lds_bytes), so that three workgroups fit a CU.
__host__ __device__ inline size_t solo_eval_lds_bytes(const SoloGeom &g) { return ((size_t)g.o_vec + 2 * (size_t)g.DSS) * sizeof(double) + 64; }

// one point per workgroup, nothing else: the form that measured 8.0 us per launch at B = 1 (the grid-stride form below: 9.5)
__global__ __launch_bounds__(SOLO_NT) void solo_eval_one_kernel(const DevProblem *__restrict__ Pp, SoloGeom g, const double *theta,
                                                                const int *spec, int jacobian, double *lp, double *grad)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const DevProblem &P = *Pp;
    const int tid = threadIdx.x, b = blockIdx.x;
    double *TH = smem + g.o_vec, *GR = TH + g.DSS, *lps = smem + g.o_scv + 12;
    if (tid < g.DSS) { TH[tid] = tid < g.D ? theta[(size_t)b * g.D + tid] : 0.0; GR[tid] = 0.0; }
    solo_eval_init(P, g, smem, tid);
    const SoloEvalRegs er = solo_eval_setup(P, g, spec ? spec[b] : 0, tid);
    __syncthreads();
    solo_eval(P, g, smem, TH, GR, lps, er, jacobian, tid);
    if (tid < g.D && grad) grad[(size_t)b * g.D + tid] = GR[tid];
    if (tid == 0 && lp) lp[b] = *lps;
}

// TIGHT: 80 VGPRs (six waves per SIMD: three workgroups share a CU) for batches of more points than CUs
template <bool TIGHT>
__global__ __launch_bounds__(SOLO_NT, TIGHT ? 6 : 2) void solo_eval_kernel(const DevProblem *__restrict__ Pp, SoloGeom g, const double *theta,
                                                                          const int *spec, int B, int jacobian, double *lp, double *grad)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const DevProblem &P = *Pp;
    const int tid = threadIdx.x;
    double *TH = smem + g.o_vec, *GR = TH + g.DSS, *lps = smem + g.o_scv + 12;
    solo_eval_init(P, g, smem, tid);
    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        if (tid < g.DSS) { TH[tid] = tid < g.D ? theta[(size_t)b * g.D + tid] : 0.0; GR[tid] = 0.0; }
        const SoloEvalRegs er = solo_eval_setup(P, g, spec ? spec[b] : 0, tid);
        __syncthreads();
        solo_eval<TIGHT ? 8 : 16>(P, g, smem, TH, GR, lps, er, jacobian, tid);
        if (tid < g.D && grad) grad[(size_t)b * g.D + tid] = GR[tid];
        if (tid == 0 && lp) lp[b] = *lps;
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// One chain per workgroup, general block model (bdrt_solo_wide.h): the evaluation by 512 threads, everything after it by the
// cooperative stage of bdrt_nuts_wide.h.  Global state layout: vecs [n_units][V_COUNT][ds] (the rows of nuts_kernel, one column).
// ---------------------------------------------------------------------------------------------------------------------------
// rows of the chain kept in LDS for the launch, most used first (as many as fit: `nhot`): a plain leaf then touches HBM only
// for the trajectory ends / higher checkpoint levels it rarely needs
__device__ __constant__ signed char W1_HOT_ORDER[12] = {V_TH, V_P, V_G, V_MINV, V_CKP, V_THQ, V_GQ, V_CKP + 1, V_CKC + 1, V_CKP + 2, V_CKC + 2, V_RHO};

template <bool PROF = false>
__global__ __launch_bounds__(SOLO_NT) void nuts_wide1_kernel(const DevProblem *__restrict__ Pp, NutsParams np, NutsArgs a, Wide1Geom G, int nhot)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const DevProblem &P = *Pp;
    const int tid = threadIdx.x;
    const int wg = blockIdx.x, unit = a.unit_map ? a.unit_map[wg] : wg;
    const int D = P.D, DS = a.ds;
    double *scr = smem + G.total;
    double *lpn = scr + W1_SCRATCH;
    double *hot = lpn + 2;                                 // [nhot][ds]
    ChainState *sts = reinterpret_cast<ChainState *>(hot + (size_t)nhot * DS);
    signed char *hslot = reinterpret_cast<signed char *>(sts + 1);      // [V_COUNT] (64 bytes)
    double *V = a.vecs + (size_t)wg * V_COUNT * DS;       // this chain's rows [V_COUNT][ds]
    auto grow = [&](int v) -> double * { return V + (size_t)v * DS; };                                    // the row in HBM
    auto row = [&](int v) -> double * { const int h = hslot[v]; return h >= 0 ? hot + (size_t)h * DS : grow(v); };
    if (tid == 0) chain_state_copy(sts[0], a.states[unit]);
    if (tid < V_COUNT) {
        int h = -1;
        for (int k = 0; k < nhot; ++k) if (W1_HOT_ORDER[k] == tid) h = k;
        hslot[tid] = (signed char)h;
    }
    wide1_init(P, G, smem, tid);
    for (int k = 0; k < nhot; ++k) {
        const double *src = grow(W1_HOT_ORDER[k]);
        for (int j = tid; j < DS; j += SOLO_NT) hot[(size_t)k * DS + j] = src[j];
    }
    __syncthreads();
    const SoloEvalRegs er = solo_eval_setup(P, G.g, sts[0].spec, tid);
    if (!sts[0].kicked) {
        // half kick + drift of the first evaluation of a freshly created sampler
        const int ph = sts[0].phase;
        const double e = ph == PH_EPS ? sts[0].eps : (ph == PH_TREE ? sts[0].dir * sts[0].eps : 0.0);
        double *TH = row(V_TH), *Pm = row(V_P), *Gr = row(V_G), *MI = row(V_MINV);
        if (ph == PH_INIT || ph == PH_EPS || ph == PH_TREE)
            for (int j = tid; j < D; j += SOLO_NT) {
                const double p = Pm[j] + 0.5 * e * Gr[j];
                Pm[j] = p;
                TH[j] += e * MI[j] * p;
            }
        __syncthreads();
        if (tid == 0) sts[0].kicked = 1;
        __syncthreads();
    }
    WideCtx wx;
    wx.P = Pp; wx.np = &np; wx.a = &a; wx.V = V; wx.smem = scr; wx.sts = sts; wx.lpn = lpn; wx.hvy = nullptr; wx.hvk = nullptr;
    wx.prof = nullptr; wx.D = D; wx.DS = DS; wx.TH2OFF = 0; wx.c0 = unit; wx.nvalid = 1; wx.slot_unit = nullptr; wx.ncol = 1;
    wx.hot_base = hot; wx.hot_slot = hslot;
    unsigned long long my_leaps = 0;
    for (int round = 0; round < a.rounds; ++round) {
        const int ph = sts[0].phase;
        if (!(ph == PH_INIT || ph == PH_EPS || ph == PH_TREE)) break;
        long long *prof = (PROF && a.prof) ? a.prof + (size_t)wg * 32 : nullptr;       // slots 0 / 1: evaluation / everything after it (thread 0)
        const long long t0 = (prof && tid == 0) ? clock64() : 0;
        wide1_eval(P, G, smem, row(V_TH), row(V_G), lpn, er, 1, tid, prof);
        const long long t1 = (prof && tid == 0) ? clock64() : 0;
        wx.prof = prof ? prof + 16 : nullptr;                                // (slots 25, 27..31: the stages of the cooperative tail)
        wide_coop_tail<2, true>(wx, 0, false, my_leaps, tid);
        __syncthreads();
        if (prof && tid == 0) { prof[0] += t1 - t0; prof[1] += clock64() - t1; }
    }
    // the LDS-resident rows go back to the chain's HBM rows
    for (int k = 0; k < nhot; ++k) {
        double *dst = grow(W1_HOT_ORDER[k]);
        for (int j = tid; j < DS; j += SOLO_NT) dst[j] = hot[(size_t)k * DS + j];
    }
    if (tid == 0) {
        chain_state_copy(a.states[unit], sts[0]);
        if (my_leaps) atomicAdd(a.leap_counter, my_leaps);
        const int ph = sts[0].phase;
        if (!(ph == PH_INIT || ph == PH_EPS || ph == PH_TREE)) atomicAdd(a.done_counter, 1);
    }
}

// the general one-chain evaluator (bdrt_solo_wide.h) on its own: one point per workgroup (tests)
// ---------------------------------------------------------------------------------------------------------------------------
// Problems beyond the LDS budget (bdrt_big.h): one chain per workgroup, every row of the chain in HBM, the evaluation by the
// streamed evaluator (workspace in HBM), everything after it by the cooperative stage of bdrt_nuts_wide.h.  Slow but working:
// the reference accepts any grid (inversion.py:2127-2209).  State layout: that of nuts_wide1_kernel.
// ---------------------------------------------------------------------------------------------------------------------------
// NJX: elements of a parameter vector per thread of the cooperative stage, D <= 512 NJX (2: D <= 1024; 4: D <= 2048 -- three
// distributions of 301 basis functions are 1821 parameters; 8 and 16: D <= 4096 / 8192, one distribution of 1200 basis functions
// is 2409 -- these two keep most of the stage's rows in scratch memory: the streamed path is the slow path either way).  The
// stage's LDS scratch holds the D momentum normals behind its 512 doubles of reduction scratch.

template <int NJX>
__global__ __launch_bounds__(SOLO_NT) void nuts_big_kernel(const DevProblem *__restrict__ Pp, NutsParams np, NutsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const DevProblem &P = *Pp;
    const int tid = threadIdx.x;
    const int wg = blockIdx.x, unit = a.unit_map ? a.unit_map[wg] : wg;
    const int D = P.D, DS = a.ds;
    double *scr = smem;
    double *lpn = scr + big_scratch_doubles(NJX);
    double *red = lpn + 2;
    ChainState *sts = reinterpret_cast<ChainState *>(red + 9 * 8);
    signed char *hslot = reinterpret_cast<signed char *>(sts + 1);      // [V_COUNT] (64 bytes): no row is LDS-resident
    double *V = a.vecs + (size_t)wg * V_COUNT * DS;       // this chain's rows [V_COUNT][ds]
    double *ws = a.bigws + (size_t)wg * big_ws_doubles(P);
    auto row = [&](int v) -> double * { return V + (size_t)v * DS; };
    if (tid == 0) chain_state_copy(sts[0], a.states[unit]);
    if (tid < V_COUNT) hslot[tid] = (signed char)-1;
    __syncthreads();
    const int spec = sts[0].spec;
    if (!sts[0].kicked) {
        const int ph = sts[0].phase;
        const double e = ph == PH_EPS ? sts[0].eps : (ph == PH_TREE ? sts[0].dir * sts[0].eps : 0.0);
        double *TH = row(V_TH), *Pm = row(V_P), *Gr = row(V_G), *MI = row(V_MINV);
        if (ph == PH_INIT || ph == PH_EPS || ph == PH_TREE)
            for (int j = tid; j < D; j += SOLO_NT) {
                const double p = Pm[j] + 0.5 * e * Gr[j];
                Pm[j] = p;
                TH[j] += e * MI[j] * p;
            }
        __syncthreads();
        if (tid == 0) sts[0].kicked = 1;
        __syncthreads();
    }
    WideCtx wx;
    wx.P = Pp; wx.np = &np; wx.a = &a; wx.V = V; wx.smem = scr; wx.sts = sts; wx.lpn = lpn; wx.hvy = nullptr; wx.hvk = nullptr;
    wx.prof = nullptr; wx.D = D; wx.DS = DS; wx.TH2OFF = 0; wx.c0 = unit; wx.nvalid = 1; wx.slot_unit = nullptr; wx.ncol = 1;
    wx.hot_base = scr; wx.hot_slot = hslot;
    unsigned long long my_leaps = 0;
    for (int round = 0; round < a.rounds; ++round) {
        const int ph = sts[0].phase;
        if (!(ph == PH_INIT || ph == PH_EPS || ph == PH_TREE)) break;
        // the rows of the last cooperative stage (global stores of other threads) are read by this evaluation
        __threadfence_block();
        __syncthreads();
        big_eval(P, ws, row(V_TH), row(V_G), lpn, spec, 1, red, tid);
        __threadfence_block();
        __syncthreads();
        wide_coop_tail<NJX, true>(wx, 0, false, my_leaps, tid);
        __syncthreads();
    }
    if (tid == 0) {
        chain_state_copy(a.states[unit], sts[0]);
        if (my_leaps) atomicAdd(a.leap_counter, my_leaps);
        const int ph = sts[0].phase;
        if (!(ph == PH_INIT || ph == PH_EPS || ph == PH_TREE)) atomicAdd(a.done_counter, 1);
    }
}

__global__ __launch_bounds__(SOLO_NT) void wide1_eval_kernel(const DevProblem *__restrict__ Pp, Wide1Geom G, const double *theta,
                                                             const int *spec, int B, int jacobian, double *lp, double *grad)
{
    extern __shared__ __attribute__((aligned(16))) double smem[];
    const DevProblem &P = *Pp;
    const int tid = threadIdx.x;
    wide1_init(P, G, smem, tid);
    for (int b = blockIdx.x; b < B; b += gridDim.x) {          // (a workgroup per point, or a grid-stride loop over the points)
        const SoloEvalRegs er = solo_eval_setup(P, G.g, spec ? spec[b] : 0, tid);
        __syncthreads();
        wide1_eval(P, G, smem, theta + (size_t)b * P.D, grad + (size_t)b * P.D, lp + b, er, jacobian, tid);
    }
}


// Hand-over of the tail of a large run (bdrt_sampler.hip: maybe_migrate_tail): copies a live chain's rows from the 16-chain layout
// [wg][V_*][column][ds16] to the one-chain layout [slot][SV_* / SG_*][dss].  Same counter-based random numbers and the same
// arithmetic up to summation order, so the chains continue as they were.
__global__ void nuts_migrate_kernel(const double *v16, int ds16, const int *unit_loc, const int *unit_map, double *vsolo, int dss, int D)
{
    const int slot = blockIdx.x, u = unit_map[slot];
    const int wg = unit_loc[u] >> 4, col = slot_col(unit_loc[u] & 15);      // where the unit sits in the 16-chain layout
    const double *src = v16 + (size_t)wg * V_COUNT * NC * ds16;
    double *dst = vsolo + (size_t)slot * SG_COUNT * dss;
    for (int r = 0; r < SG_COUNT; ++r) {
        int v;                                            // row of the 16-chain layout that holds row r of the solo layout
        if (r < SV_CKC) { constexpr int head[SV_CKC] = {V_TH, V_P, V_G, V_THM, V_PM, V_GM, V_THP, V_PP, V_GP, V_THS, V_GS, V_THQ, V_GQ, V_RHO, V_MINV}; v = head[r]; }
        else if (r < SV_CKP) v = V_CKC + (r - SV_CKC);
        else if (r < SV_COUNT) v = V_CKP + (r - SV_CKP);
        else v = r == SG_WMEAN ? V_WMEAN : V_WM2;
        const double *sr = src + ((size_t)v * NC + col) * ds16;
        for (int j = threadIdx.x; j < dss; j += blockDim.x) dst[(size_t)r * dss + j] = j < D ? sr[j] : 0.0;
    }
}
static_assert(SOLO_MAXD == MAXD, "the two kernels keep the same number of checkpoint levels");

// the same hand-over for the models of the general one-chain kernel (bdrt_solo_wide.h): rows keep their meaning, the chain's
// column of [wg][V_*][16][ds] becomes [slot][V_*][ds]
__global__ void nuts_migrate_wide1_kernel(const double *v16, int ds, const int *unit_loc, const int *unit_map, double *v1, ChainState *states)
{
    const int slot = blockIdx.x, u = unit_map[slot];
    const int wg = unit_loc[u] >> 4, col = slot_col(unit_loc[u] & 15);
    const double *src = v16 + (size_t)wg * V_COUNT * NC * ds;
    double *dst = v1 + (size_t)slot * V_COUNT * ds;
    const int live = states[u].thsel ? V_TH2 : V_TH;       // the one-chain kernel keeps theta in V_TH
    for (int v = 0; v < V_COUNT; ++v) {
        const int sv = v == V_TH ? live : v;
        for (int j = threadIdx.x; j < ds; j += blockDim.x) dst[(size_t)v * ds + j] = src[((size_t)sv * NC + col) * ds + j];
    }
    __syncthreads();
    if (threadIdx.x == 0) states[u].thsel = 0;
}

// Compaction of a large run (bdrt_sampler.hip: maybe_compact): workgroup `blockIdx.x` of the NEW layout gathers the rows of its up
// to 16 units from wherever they sat in the old one.  Rows are copied verbatim and every random number is keyed by (seed, chain id,
// iteration, ...), never by the slot, so the chains continue bit for bit (tests/test_gpu_config4.py).  Empty slots get the finite
// placeholders of a fresh sampler (inverse metric 1, zeros elsewhere).
__global__ __launch_bounds__(256) void nuts_compact_kernel(const double *vold, const int *old_loc, const int *new_slot_unit,
                                                           double *vnew, int ds)
{
    const int wg = blockIdx.x;
    const size_t rowlen = (size_t)ds;
    for (int k = 0; k < NC; ++k) {
        const int u = new_slot_unit[wg * NC + k];
        const int col = slot_col(k);
        double *dst = vnew + (size_t)wg * V_COUNT * NC * rowlen;
        if (u < 0) {
            for (int v = 0; v < V_COUNT; ++v)
                for (int j = threadIdx.x; j < ds; j += blockDim.x) dst[((size_t)v * NC + col) * rowlen + j] = v == V_MINV ? 1.0 : 0.0;
            continue;
        }
        const int owg = old_loc[u] >> 4, ocol = slot_col(old_loc[u] & 15);
        const double *src = vold + (size_t)owg * V_COUNT * NC * rowlen;
        for (int v = 0; v < V_COUNT; ++v)
            for (int j = threadIdx.x; j < ds; j += blockDim.x)
                dst[((size_t)v * NC + col) * rowlen + j] = src[((size_t)v * NC + ocol) * rowlen + j];
    }
}

// liveness of every unit (1: the chain is still running), for the host's re-packing decision
__global__ void nuts_live_kernel(const ChainState *states, int n, int *live)
{
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u < n) { const int ph = states[u].phase; live[u] = (ph == PH_INIT || ph == PH_EPS || ph == PH_TREE) ? 1 : 0; }
}

// any_b: the caller wants ONE evaluator whatever the batch size (the Newton iteration's trial points: a fit's numbers must not depend on
// how many other fits share its batch) -- the headline family's one-workgroup-per-point evaluator then takes any B (grid-stride), every
// other family answers 1 (the caller's tile evaluator, also for every B)
int launch_logp_grad_few(Problem *p, const double *d_theta, const int *d_spec, int B, int jacobian, double *d_lp, double *d_grad,
                         hipStream_t stream, int any_b)
{
    Problem &P = *p;
    const char *sw = getenv("BDRT_FEW_POINTS");                     // diagnostics / tests: 0 = the tile evaluator whatever B is
    const bool off = sw && atoi(sw) == 0;
    if (off || B < 1 || !d_grad || !d_lp) return 1;
    if (P.few_kind < 0) {
        P.few_kind = solo_capable(P.dev) ? 1 : (wide1_capable(P.dev) ? 2 : 0);
        hipDeviceProp_t prop;
        P.few_ncu = (hipGetDeviceProperties(&prop, P.device) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    }
    if (P.few_kind == 0) return 1;
    const bool solo = P.few_kind == 1;
    const int ncu = P.few_ncu;
    BDRT_HIP(hipSetDevice(P.device));
    // a few points per CU: beyond that the 16-column tiles win (26 us up to 16 points per CU).  BDRT_FEW_POINTS=n: n points per CU
    // at most (default 5 for the LDS-light evaluator of the headline family, three workgroups of which share a CU; 1 otherwise)
    const int per_cu = sw ? atoi(sw) : (solo ? 5 : 1);
    if (any_b ? !solo : B > per_cu * ncu) return 1;
    static LdsAttrCache attr_solo, attr_w1;
    if (solo) {
        const SoloGeom g = solo_geometry(P.dev.nf, P.dev.blk[0].K, P.dev.D);
        // The LDS request doubles as a placement hint: the dispatcher packs as many workgroups on a CU as their resources allow
        // and leaves other CUs idle, so each workgroup asks for its share of a CU -- all of it while there are at most as many
        // points as CUs (measured: 8.0 us at B = 1 against 9.5 us when three fit), half or a third beyond
        const int wgs = B <= ncu ? B : std::min(B, 3 * ncu);
        const int share = std::min(3, (wgs + ncu - 1) / ncu);
        const size_t lds = std::max(solo_eval_lds_bytes(g), (size_t)(160 * 1024) / share - 2048);
        const size_t lds_max = (size_t)160 * 1024 - 2048;
        BDRT_HIP(attr_solo.ensure(lds_max, [&]() {
            hipError_t e = hipFuncSetAttribute((const void *)solo_eval_one_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
            if (e == hipSuccess) e = hipFuncSetAttribute((const void *)solo_eval_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max);
            return e; }));
        if (B <= ncu)
            hipLaunchKernelGGL(solo_eval_one_kernel, dim3(wgs), dim3(SOLO_NT), (size_t)g.total * sizeof(double) + 64, stream, (const DevProblem *)P.d_dev, g,
                               d_theta, d_spec, jacobian, d_lp, d_grad);
        else
            hipLaunchKernelGGL(solo_eval_kernel<true>, dim3(wgs), dim3(SOLO_NT), lds, stream, (const DevProblem *)P.d_dev, g,
                               d_theta, d_spec, B, jacobian, d_lp, d_grad);
    } else {
        const Wide1Geom G = wide1_geometry(P.dev.nf, P.dev.blk[0].K, P.dev.D, P.dev.nblocks);
        const size_t lds = (size_t)G.total * sizeof(double) + 64;
        BDRT_HIP(attr_w1.ensure(lds, [&]() {
            return hipFuncSetAttribute((const void *)wide1_eval_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); }));
        const int wgs = std::min(B, 2 * ncu);
        hipLaunchKernelGGL(wide1_eval_kernel, dim3(wgs), dim3(SOLO_NT), lds, stream, (const DevProblem *)P.d_dev, G, d_theta, d_spec, B,
                           jacobian, d_lp, d_grad);
    }
    BDRT_HIP(hipGetLastError());
    return 0;
}

// The Stan-style L-BFGS of n fits as one launch (bdrt_lbfgs_dev.h).  Returns 1 when the problem takes neither one-chain
// evaluator (caller: host-driven path), 0 on success (x_out / g_out [n][D]: last iterate and the gradient of -lp there).
int lbfgs_device(Problem &P, const double *x0, const int *spec, int n, const bdrt_opt_options &o, double *x_out, double *g_out,
                 int *iters, int *n_evals, int *rc, double *f)
{
    const bool solo = solo_capable(P.dev), w1 = !solo && wide1_capable(P.dev);
    if ((!solo && !w1) || n < 1 || o.history > LBFGS_MAX_HISTORY) return 1;
    BDRT_HIP(hipSetDevice(P.device));
    const int D = P.dev.D;
    SoloGeom g = solo_geometry(P.dev.nf, P.dev.blk[0].K, D);
    Wide1Geom G = wide1_geometry(P.dev.nf, P.dev.blk[0].K, D, P.dev.nblocks);
    const int DS = (D + 7) & ~7;
    size_t lds;
    if (solo) {
        lds = ((size_t)g.o_vec + (size_t)(2 + 2 * LBFGS_MAX_HISTORY) * g.DSS) * sizeof(double) + 64;
        if (lds > 160 * 1024) return 1;
    } else {
        lds = ((size_t)G.total + 8) * sizeof(double) + 64;
    }
    DevBuf<double> dx0, dxo, dgo, dwork;
    DevBuf<LbfgsDevReport> drep;
    DevBuf<int> dspec;
    const size_t nD = (size_t)n * D;
    if (upload(dx0, x0, nD) || (spec && upload(dspec, spec, (size_t)n))) return -10;
    BDRT_HIP(dxo.alloc(nD)); BDRT_HIP(dgo.alloc(nD));
    BDRT_HIP(drep.alloc((size_t)n));
    if (!solo) BDRT_HIP(dwork.alloc((size_t)n * LBFGS_WIDE_ROWS * DS));
    const long long cap = (long long)std::max(o.max_iter, 0) * 4 + 64;
    const int max_evals = (int)std::min<long long>(cap, 1LL << 30);
    static LdsAttrCache attr_s, attr_w;
    if (solo) {
        BDRT_HIP(attr_s.ensure(lds, [&]() { return hipFuncSetAttribute((const void *)lbfgs_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); }));
        hipLaunchKernelGGL(lbfgs_kernel<false>, dim3(n), dim3(SOLO_NT), lds, P.stream, (const DevProblem *)P.d_dev, g, G, (const double *)dx0.p,
                           (const int *)dspec.p, o, max_evals, (double *)dxo.p, (double *)dgo.p, (LbfgsDevReport *)drep.p, (double *)nullptr, DS);
    } else {
        BDRT_HIP(attr_w.ensure(lds, [&]() { return hipFuncSetAttribute((const void *)lbfgs_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); }));
        hipLaunchKernelGGL(lbfgs_kernel<true>, dim3(n), dim3(SOLO_NT), lds, P.stream, (const DevProblem *)P.d_dev, g, G, (const double *)dx0.p,
                           (const int *)dspec.p, o, max_evals, (double *)dxo.p, (double *)dgo.p, (LbfgsDevReport *)drep.p, (double *)dwork.p, DS);
    }
    BDRT_HIP(hipGetLastError());
    BDRT_HIP(hipStreamSynchronize(P.stream));
    std::vector<LbfgsDevReport> reps((size_t)n);
    if (download(reps.data(), drep.p, reps.size()) || download(x_out, dxo.p, nD) || download(g_out, dgo.p, nD)) return -10;
    for (int i = 0; i < n; ++i) { iters[i] = reps[i].iters; n_evals[i] = reps[i].n_evals; rc[i] = reps[i].rc; f[i] = reps[i].f; }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Launchers (bdrt_nuts_launch.h).  ONE table holds every sampler instantiation under its key; its 16-chain part IS the list of
// bdrt_nuts16.h (BDRT_NUTS16_G0..G5): an instantiation added to a group can be launched and has its LDS limit raised, a key in
// no group is an error.  (The table stands AFTER the evaluator / L-BFGS launchers above and names the one-chain kernels in this
// order on purpose: templates are instantiated in the order of first use, and lbfgs_kernel<true> compiles differently otherwise.)
// ---------------------------------------------------------------------------------------------------------------------------
struct NutsEntry {
    NutsKey key;
    bool prof;
    int n_threads;
    const void *fn;
};
#define BDRT_NUTS16_ENTRY(NJ_, MODE_, TA_) {{NutsFamily::tile16, NJ_, MODE_, TA_}, false, NT, (const void *)nuts_kernel<NJ_, MODE_, TA_, false>},
#define BDRT_NUTS16_ENTRY_PROF(NJ_, MODE_, TA_) {{NutsFamily::tile16, NJ_, MODE_, TA_}, true, NT, (const void *)nuts_kernel<NJ_, MODE_, TA_, true>},
#define BDRT_NUTS1_ENTRY(FAMILY_, A_, PROF_, ...) {{NutsFamily::FAMILY_, A_, 0, 0}, PROF_, SOLO_NT, (const void *)__VA_ARGS__},
static const NutsEntry nuts_table[] = {
    BDRT_NUTS1_ENTRY(solo, 2, false, nuts_solo_kernel<2, false>) BDRT_NUTS1_ENTRY(solo, 4, false, nuts_solo_kernel<4, false>)
    BDRT_NUTS1_ENTRY(solo, 2, true, nuts_solo_kernel<2, true>) BDRT_NUTS1_ENTRY(solo, 4, true, nuts_solo_kernel<4, true>)
    BDRT_NUTS1_ENTRY(wide1, 0, false, nuts_wide1_kernel<false>) BDRT_NUTS1_ENTRY(wide1, 0, true, nuts_wide1_kernel<true>)
    BDRT_NUTS1_ENTRY(big, 2, false, nuts_big_kernel<2>) BDRT_NUTS1_ENTRY(big, 4, false, nuts_big_kernel<4>)
    BDRT_NUTS1_ENTRY(big, 8, false, nuts_big_kernel<8>) BDRT_NUTS1_ENTRY(big, 16, false, nuts_big_kernel<16>)
    BDRT_NUTS16_G0(BDRT_NUTS16_ENTRY) BDRT_NUTS16_G1(BDRT_NUTS16_ENTRY) BDRT_NUTS16_G2(BDRT_NUTS16_ENTRY)
    BDRT_NUTS16_G3(BDRT_NUTS16_ENTRY) BDRT_NUTS16_G4(BDRT_NUTS16_ENTRY) BDRT_NUTS16_G5(BDRT_NUTS16_ENTRY_PROF)};
#undef BDRT_NUTS16_ENTRY
#undef BDRT_NUTS16_ENTRY_PROF
#undef BDRT_NUTS1_ENTRY

hipError_t nuts_set_lds_limit(size_t bytes)
{
    static LdsAttrCache cache;
    return cache.ensure(bytes, [&]() {
        hipError_t e = hipSuccess;
        for (const auto &k : nuts_table)              // (the streamed kernels keep the default limit)
            if (e == hipSuccess && k.key.family != NutsFamily::big) e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        return e;
    });
}

int launch_nuts(NutsKey key, const DevProblem *dp, const NutsParams &np, const NutsArgs &args, int n_wg, size_t lds, hipStream_t stream,
                const void *extra0, const void *extra1)
{
    const NutsEntry *plain = nullptr, *prof = nullptr;
    for (const auto &k : nuts_table)
        if (k.key.family == key.family && k.key.a == key.a && k.key.b == key.b && k.key.c == key.c) (k.prof ? prof : plain) = &k;
    if (!plain) { set_error("no sampler kernel of family %d with key <%d, %d, %d>", (int)key.family, key.a, key.b, key.c); return -11; }
    void *argv[] = {(void *)&dp, (void *)&np, (void *)&args, (void *)extra0, (void *)extra1};
    const NutsEntry &k = args.prof && prof ? *prof : *plain;
    BDRT_HIP(hipLaunchKernel(k.fn, dim3(n_wg), dim3(k.n_threads), argv, lds, stream));
    return 0;
}

int launch_nuts_live(const ChainState *states, int n_units, int *live, hipStream_t stream)
{
    hipLaunchKernelGGL(nuts_live_kernel, dim3((n_units + 255) / 256), dim3(256), 0, stream, states, n_units, live);
    BDRT_HIP(hipGetLastError());
    return 0;
}

int launch_nuts_migrate(bool to_solo, const double *v16, int ds16, const int *unit_loc, const int *unit_map, int n_tail, double *vnew, int dss,
                        int D, ChainState *states, hipStream_t stream)
{
    if (to_solo) hipLaunchKernelGGL(nuts_migrate_kernel, dim3((unsigned)n_tail), dim3(256), 0, stream, v16, ds16, unit_loc, unit_map, vnew, dss, D);
    else hipLaunchKernelGGL(nuts_migrate_wide1_kernel, dim3((unsigned)n_tail), dim3(256), 0, stream, v16, ds16, unit_loc, unit_map, vnew, states);
    BDRT_HIP(hipGetLastError());
    return 0;
}

int launch_nuts_compact(const double *vold, const int *old_loc, const int *new_slot_unit, int n_wg, double *vnew, int ds, hipStream_t stream)
{
    hipLaunchKernelGGL(nuts_compact_kernel, dim3(n_wg), dim3(256), 0, stream, vold, old_loc, new_slot_unit, vnew, ds);
    BDRT_HIP(hipGetLastError());
    return 0;
}

}  // namespace bdrt

using namespace bdrt;

// test probe (tests/test_gpu_lean_math.py): a leaf's acceptance decision and new log-weight in the device form of nuts_leaf_joins (one
// exponential) and in the textbook form (log_sum_exp2, u < exp(w - lsw_new)) -- both with the device's lean exp / log
__global__ void leaf_joins_probe_kernel(const double *lsw_sub, const double *w, const double *u, int n, double *lsw_dev, int *join_dev,
                                        double *lsw_ref, int *join_ref, double *prob_ref)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double l;
    join_dev[i] = nuts_leaf_joins(lsw_sub[i], w[i], u[i], l) ? 1 : 0;
    lsw_dev[i] = l;
    const double lr = log_sum_exp2(lsw_sub[i], w[i]);
    const double pr = BDRT_NUTS_EXP(w[i] - lr);
    lsw_ref[i] = lr; prob_ref[i] = pr; join_ref[i] = u[i] < pr ? 1 : 0;
}

extern "C" {

/* parity-test hooks (not part of include/bdrt.h): one of the one-chain evaluators on B points -- the one-chain-per-workgroup path's
   (bdrt_solo.h), the one-chain-per-wave path's (bdrt_wave.h), the general one (bdrt_solo_wide.h) */
enum class DebugEval { solo, wave, wide1 };
static int debug_logp_grad(DebugEval which, const char *who, bdrt_problem *p, const double *theta, const int *spec, int B, int jacobian,
                           double *lp, double *grad)
{
    if (!p || !theta || B < 1) { set_error("%s: bad arguments", who); return -1; }
    Problem &P = p->impl;
    const DevProblem *dp = (const DevProblem *)P.d_dev;
    if (which == DebugEval::solo && !solo_capable(P.dev)) { set_error("problem does not take the solo path"); return -2; }
    if (which == DebugEval::wave && !wave_capable(P.dev)) { set_error("problem does not take the one-chain-per-wave path"); return -2; }
    if (which == DebugEval::wide1 && !wide1_capable(P.dev)) { set_error("problem does not take the general one-chain evaluator"); return -2; }
    BDRT_HIP(hipSetDevice(P.device));
    DevBuf<double> dth, dlp, dg;
    DevBuf<int> dsp;
    const size_t n = (size_t)B * P.dev.D;
    if (upload(dth, theta, n) || (spec && upload(dsp, spec, (size_t)B))) return -10;
    BDRT_HIP(dg.alloc(n)); BDRT_HIP(dlp.alloc(B));
    BDRT_HIP(hipMemset(dg, 0, n * sizeof(double)));
    if (which == DebugEval::solo) {
        const SoloGeom g = solo_geometry(P.dev.nf, P.dev.blk[0].K, P.dev.D);
        const size_t lds = solo_eval_lds_bytes(g);
        BDRT_HIP(hipFuncSetAttribute((const void *)solo_eval_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(solo_eval_kernel<false>, dim3(B), dim3(SOLO_NT), lds, 0, dp, g, dth.p, dsp.p, B, jacobian, dlp.p, dg.p);
    } else if (which == DebugEval::wave) {
        const WaveGeom g = wave_geometry(P.dev.nf, P.dev.blk[0].K, P.dev.D, P.dev.nblocks);
        if (const int rc = launch_wave_eval(dp, g, dth, dsp, B, jacobian, dlp, dg, std::min(B, 2048), wave_lds_bytes(g, 0), 0, P.dev.outlier_mode != 0)) return rc;
    } else {
        const Wide1Geom G = wide1_geometry(P.dev.nf, P.dev.blk[0].K, P.dev.D, P.dev.nblocks);
        const size_t lds = (size_t)G.total * sizeof(double) + 64;
        BDRT_HIP(hipFuncSetAttribute((const void *)wide1_eval_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(wide1_eval_kernel, dim3(B), dim3(SOLO_NT), lds, 0, dp, G, dth.p, dsp.p, B, jacobian, dlp.p, dg.p);
    }
    BDRT_HIP(hipGetLastError());
    BDRT_HIP(hipDeviceSynchronize());
    if ((lp && download(lp, dlp.p, (size_t)B)) || (grad && download(grad, dg.p, n))) return -10;
    return 0;
}
int bdrt_debug_solo_logp_grad(bdrt_problem *p, const double *theta, const int *spec, int B, int jacobian, double *lp, double *grad)
{
    return debug_logp_grad(DebugEval::solo, "bdrt_debug_solo_logp_grad", p, theta, spec, B, jacobian, lp, grad);
}
int bdrt_debug_wave_logp_grad(bdrt_problem *p, const double *theta, const int *spec, int B, int jacobian, double *lp, double *grad)
{
    return debug_logp_grad(DebugEval::wave, "bdrt_debug_wave_logp_grad", p, theta, spec, B, jacobian, lp, grad);
}
int bdrt_debug_wide1_logp_grad(bdrt_problem *p, const double *theta, const int *spec, int B, int jacobian, double *lp, double *grad)
{
    return debug_logp_grad(DebugEval::wide1, "bdrt_debug_wide1_logp_grad", p, theta, spec, B, jacobian, lp, grad);
}

int bdrt_debug_leaf_joins(const double *lsw_sub, const double *w, const double *u, int n, double *lsw_dev, int *join_dev, double *lsw_ref,
                          int *join_ref, double *prob_ref)
{
    if (!lsw_sub || !w || !u || !lsw_dev || !join_dev || !lsw_ref || !join_ref || !prob_ref || n < 1) {
        set_error("bdrt_debug_leaf_joins: bad arguments"); return -1;
    }
    DevBuf<double> d[6];
    DevBuf<int> di[2];
    const size_t N = (size_t)n;
    if (upload(d[0], lsw_sub, N) || upload(d[1], w, N) || upload(d[2], u, N)) return -10;
    for (int k = 3; k < 6; ++k) BDRT_HIP(d[k].alloc(N));
    for (auto &q : di) BDRT_HIP(q.alloc(N));
    hipLaunchKernelGGL(leaf_joins_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, d[0].p, d[1].p, d[2].p, n, d[3].p, di[0].p, d[4].p, di[1].p, d[5].p);
    BDRT_HIP(hipGetLastError());
    if (download(lsw_dev, d[3].p, N) || download(join_dev, di[0].p, N) || download(lsw_ref, d[4].p, N) || download(join_ref, di[1].p, N) ||
        download(prob_ref, d[5].p, N))
        return -10;
    return 0;
}

}  // extern "C"
