// bdrt_sampler.hip -- the host side of the device-resident NUTS sampler (bdrt_sampler_* of include/bdrt.h; replaces StanModel.sampling,
// reference bayes_drt/inversion.py:1218-1221).  No kernel lives here (bdrt_nuts_launch.h).  ONE value, the SamplerPlan, says which
// kernel advances a run and with what: make_plan at creation, tail migration and compaction between launches.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

#include "bdrt_nuts_launch.h"

namespace bdrt {

enum class Layout {       // state rows in HBM
    tile16,               // [wg][V_COUNT][16][ds]: sixteen chains per workgroup
    solo,                 // [unit][SG_COUNT][dss]: one chain, the rows of bdrt_solo.h (512-thread and one-chain-per-wave kernels)
    wide                  // [unit][V_COUNT][ds]: one chain, the rows of the 16-chain kernel, one column (bdrt_solo_wide.h, bdrt_big.h)
};
enum class Kernel { tile16 = 0, solo = 1, wide1 = 2, wave = 3, big = 4 };     // (the codes of bdrt_sampler_kind)
enum class WaveUse { never, by_live, always };     // may the one-chain-per-wave kernel advance the solo layout (by_live: wave_pays)

// diagnostics / measurement overrides (DESIGN.md "Environment variables"); flags: -1 not set, 0, 1
struct SamplerEnv {
    int solo = -1;             // BDRT_SOLO: 1 the 512-thread one-chain kernels / 0 the 16-chain kernel, forced; either way no tail migration
    int wave = -1;             // BDRT_WAVE: 1 the wave kernel whenever the problem allows, 0 never
    int wide1 = -1;            // BDRT_WIDE1=0: never the general one-chain kernel
    int tail_migration = -1;   // BDRT_TAIL_MIGRATION=0: the run ends on the kernel it started on
    int compaction = -1;       // BDRT_COMPACTION=0: keep the 16-chain layout as created
    int solo_duo = -1;         // BDRT_SOLO_DUO: never / always two workgroups of the 512-thread one-chain kernel per CU
    int cpw = INT_MIN;         // BDRT_CHAINS_PER_WG: a forced packing (which means the 16-chain kernel); INT_MIN: not set
    bool s1_ku6 = false;       // BDRT_S1_KU=6: the K <= 192 instantiation of MODES 3 and 4 whatever K is (measurements)
};

struct SamplerPlan {
    Layout layout = Layout::tile16;
    Kernel kernel = Kernel::tile16;    // (solo layout: the kernel at full liveness; kernel_for_launch picks per launch)
    NutsKey key = {NutsFamily::tile16, 0, 0, 0};     // the instantiation of the 16-chain / solo / wide1 / big kernel (bdrt_nuts_launch.h)
    WaveUse wave = WaveUse::never;
    int cpw = 1, n_wg = 0, ds = 0;     // chains per workgroup, workgroups, row stride
    size_t lds_bytes = 0;              // dynamic LDS of the launch = the limit set for every kernel (the maximum over what migration may need later)
    int nhot = 0;                      // wide1: rows of the chain resident in LDS
    SoloGeom geom;
    WaveGeom geomw;
    Wide1Geom geom1;
    bool may_migrate = false, may_compact = false;
};

// row stride of the state vectors = 32 NJ of the 16-chain instantiation by D alone; beyond the tiles that of nuts_big_kernel<NJX>
static int row_stride(int D) { return D <= 32 * 11 ? 32 * 11 : (D <= 32 * 16 ? 32 * 16 : (D <= 32 * 27 ? 32 * 27 : 512 * big_njx(D))); }

// as many LDS-resident rows of nuts_wide1_kernel as fit under `cap` bytes beside the evaluator
static int wide1_hot_rows(const Wide1Geom &G, int ds, size_t cap)
{
    int n = W1_HOT_MAX;
    while (n > 0 && wide1_lds_bytes(G, ds, n) > cap) --n;
    return n;
}
constexpr size_t LDS_BUDGET = 160 * 1024, WIDE1_LDS_CAP = 158 * 1024;      // (160 KiB minus a margin)

static bool chain_running(int phase) { return phase == PH_INIT || phase == PH_EPS || phase == PH_TREE; }

// can two workgroups of the one-chain kernel share a CU for this problem (LDS of the trimmed variant)?
static bool solo_duo_fits(const DevProblem &P, const SamplerEnv &env) { return env.solo_duo != 0 && 2 * solo_duo_lds_bytes(solo_geometry(P.nf, P.blk[0].K, P.D)) <= LDS_BUDGET; }

// Which kernel advances the one-chain layout (state rows [unit][SG_COUNT][ds]) while `live` chains are running: the one-chain-per-
// wave kernel from more than two live chains per CU on (measured at 81 x 161, profiles/r05/kernel_sweep.txt: up to two per CU two
// 512-thread workgroups finish a round in 9.4 us; a third chain on any CU is a second turn for them, 14.6 us, against 13.1 us of
// the wave kernel), up to the eight per CU it keeps resident.  BDRT_WAVE=1 / 0: always / never.
static bool wave_pays(int live, int n_cu) { return live > 2 * n_cu; }
static int wave_max_units(int n_cu, const DevProblem &P) { return wave_chains_per_cu(P) * n_cu; }      // (a ninth chain on any CU is a second turn of the machine: 31 us per round instead of 19)

// the kernel of the next launch (advance) / of a sampler that has not been launched yet (bdrt_sampler_kind)
static Kernel kernel_for_launch(const SamplerPlan &pl, int live, int n_cu)
{
    if (pl.layout != Layout::solo) return pl.kernel;
    return pl.wave == WaveUse::always || (pl.wave == WaveUse::by_live && wave_pays(live, n_cu)) ? Kernel::wave : Kernel::solo;
}

// what the 16-chain kernel keeps beside the tile region: lp / hand-over cells, chain states, spectrum ids / offsets / flags, and
// the uniforms of sixteen leaves per chain
constexpr size_t NUTS16_SCALAR_LDS = (size_t)3 * NC * sizeof(double) + NC * sizeof(ChainState) + 3 * NC * sizeof(int) + 16 + (size_t)NC * 16 * sizeof(double);
static_assert(NUTS16_SCALAR_LDS <= SAMPLER_LDS_RESERVE,
              "bdrt_problem_create reserves SAMPLER_LDS_RESERVE bytes for what the sampler keeps beside the tile region");
static size_t nuts_lds_bytes(const DevProblem &P, bool s1)
{
    const int nj = s1_nj(P.D);
    const size_t tile = s1 ? s1_lds_doubles(P) + (size_t)NC * 32 * nj : lds_doubles(P);   // s1: + theta rows
    return tile * sizeof(double) + NUTS16_SCALAR_LDS;
}

// ---- the three layouts of a plan (make_plan at creation, maybe_migrate_tail for the tail) -----------------------------------------
// the 16-chain kernel: evaluator (MODE), instantiation, LDS and row stride
static void plan_tile16(SamplerPlan &pl, const DevProblem &P, const SamplerEnv &env)
{
    // the fast S1 kernel (theta rows resident in LDS, MODE 2) when the problem takes that path and the rows fit; else the S1 evaluator with
    // the sampler state in HBM (MODE 3: outlier parameters, K near 192); the general half-wave evaluator (MODE 4: several distributions,
    // parallel blocks); else the generic tile (MODE 1 Toeplitz operands / MODE 0)
    // (K >= s1_kmin: what the MODE 2 instantiation takes for granted about its basis; it holds whenever D = 2 K + 9, the family's layout)
    const bool use_s1 = P.fast_s1 && P.outlier_mode == 0 && P.D <= 2 * RW && P.D <= 32 * 16 && nuts_lds_bytes(P, true) <= LDS_BUDGET &&
                        P.blk[0].K >= s1_kmin(s1_nj(P.D));
    const bool s1_hbm = !use_s1 && P.fast_s1 && P.D <= 32 * 16;
    const bool hw = P.fast_hw && P.D <= 32 * 27;
    pl.lds_bytes = !(s1_hbm || hw) ? nuts_lds_bytes(P, use_s1)
                                   : (hw ? hw_lds_doubles(P) : s1_lds_doubles(P)) * sizeof(double) + NUTS16_SCALAR_LDS;
    pl.ds = use_s1 ? 32 * s1_nj(P.D) : row_stride(P.D);
    const int nj = pl.ds / 32;
    if (use_s1) {
        // TA = DevProblem::toepA where that instantiation exists (NJ 4 and 7 have none for the default shapes' table, TA 1)
        const int ta = P.toepA;
        pl.key = {NutsFamily::tile16, nj, 2, (ta == 2 || (ta == 1 && nj != 4 && nj != 7)) ? ta : 0};
    } else if (s1_hbm || hw) {
        // the evaluator's instantiation by the longest basis (3, 4 or 6 basis functions per lane)
        const int kmax = hw ? hw_kmax(P) : P.blk[0].K;
        const int ku = env.s1_ku6 ? 0 : (kmax <= 96 ? 3 : (kmax <= 128 ? 4 : 0));
        pl.key = {NutsFamily::tile16, s1_hbm && nj != 11 ? 16 : nj, s1_hbm ? 3 : 4, ku};
    } else {
        pl.key = {NutsFamily::tile16, std::min(nj, 27), P.toep_all != 0 ? 1 : 0, 0};
    }
}

// the one-chain layout of bdrt_solo.h for n_wg chains: the 512-thread kernels (where the problem takes them) and / or the wave kernel
static void plan_solo(SamplerPlan &pl, const DevProblem &P, int n_wg, int n_cu, const SamplerEnv &env)
{
    pl.layout = Layout::solo;
    pl.kernel = pl.wave == WaveUse::always ? Kernel::wave : Kernel::solo;
    pl.geom = solo_geometry(P.nf, P.blk[0].K, P.D);
    pl.cpw = 1; pl.n_wg = n_wg; pl.ds = pl.geom.DSS;
    if (solo_capable(P)) pl.lds_bytes = (size_t)pl.geom.total * sizeof(double) + 64;      // (a wave-only family keeps the 16-chain kernel's LDS limit)
    // more chains than CUs: two workgroups per CU (128 VGPRs each, 16 of the chain's rows in LDS) overlap each other's
    // latencies; with at most one chain per CU the full-LDS variant is the faster one.  BDRT_SOLO_DUO=0 / 1: never / always.
    const bool duo = 2 * solo_duo_lds_bytes(pl.geom) <= LDS_BUDGET && (env.solo_duo >= 0 ? env.solo_duo != 0 : n_wg > n_cu);
    pl.key = {NutsFamily::solo, duo ? 4 : 2, 0, 0};
    pl.may_migrate = pl.may_compact = false;
}

// the one-chain layout of the general kernel (bdrt_solo_wide.h) for n_wg chains: as many LDS-resident rows as fit under `cap`;
// big: the same rows advanced by the streamed kernel (bdrt_big.h), none of them resident
static void plan_wide(SamplerPlan &pl, const DevProblem &P, int n_wg, bool big, int ds, size_t cap)
{
    pl.layout = Layout::wide;
    pl.kernel = big ? Kernel::big : Kernel::wide1;
    pl.key = {big ? NutsFamily::big : NutsFamily::wide1, big ? big_njx(P.D) : 0, 0, 0};
    pl.cpw = 1; pl.n_wg = n_wg;
    pl.may_migrate = pl.may_compact = false;
    if (big) return;
    pl.geom1 = wide1_geometry(P.nf, P.blk[0].K, P.D, P.nblocks);
    pl.nhot = wide1_hot_rows(pl.geom1, ds, cap);
}

// The plan of a new sampler.  No HIP call, no look at the environment.  Returns 0, or 1: LDS budget exceeded, 2: D not supported (the plan is
// filled in either way; bdrt_sampler_create reports 1 before, 2 after its check of the spectrum indices).
static int make_plan(const DevProblem &P, int n_units, int n_cu, const SamplerEnv &env, SamplerPlan &pl)
{
    const bool solo_cap = solo_capable(P), wide1_cap = wide1_capable(P);
    pl = SamplerPlan();
    // few chains of the headline family on log-uniform grids: one chain per workgroup (bdrt_solo.h)
    // (measured at 81 x 161, profiles/r03/solo_duo.txt: one workgroup per CU 30.6 M evals/s, two per CU 42-45 M from 512 units on;
    //  the 16-chain kernel passes that at ~1300 units)
    bool solo = solo_cap && n_units <= (solo_duo_fits(P, env) ? 5 * n_cu : 4 * n_cu);
    // a run that starts on the 16-chain kernel may hand its last live chains to a one-chain kernel
    bool may_migrate = (solo_cap || wide1_cap || wave_capable(P)) && !solo;
    if (env.solo >= 0) { solo = solo_cap && env.solo != 0; may_migrate = false; }
    if (env.tail_migration == 0 || (env.wide1 == 0 && !solo_cap)) may_migrate = false;
    // one chain per wave (bdrt_wave.h) for the one-chain layout
    // (families without the LDS-resident one-chain kernel -- the outlier error models: up to one chain per CU the general one-chain kernel
    //  is the faster one, 12.9 against 16.9 us per round at 256 units; from there to four per CU the wave kernel, 53 against 29 M evals/s
    //  at 1024 units: profiles/r05/wave_outliers.txt)
    // (a forced packing means the 16-chain kernel; BDRT_SOLO=0 / 1: the 16-chain kernel / the 512-thread one-chain kernels, forced)
    const bool forced_cpw = env.cpw != INT_MIN;
    bool wave = wave_capable(P) && env.wave != 0 && !forced_cpw && !(env.solo >= 0 && env.wave != 1);
    if (wave && env.solo < 0 &&
        (env.wave == 1 || (n_units <= wave_max_units(n_cu, P) && (wave_pays(n_units, n_cu) || (!solo_cap && (n_units > n_cu || !wide1_cap)))))) {
        solo = true;                                            // start in the one-chain layout
        may_migrate = false;
    }
    // few chains of a model the LDS-resident kernel does not cover: still one chain per workgroup, evaluated by 512 threads
    // (measured at D = 818: 12.7 M evals/s from 256 units on; the 16-chain kernel passes that at ~750)
    const bool wide1 = !solo && n_units <= (11 * n_cu) / 4 && wide1_cap && env.wide1 != 0 && !forced_cpw;
    // a problem beyond the LDS budget of the tile evaluators (bdrt_big.h): one chain per workgroup in the same row layout, the
    // streamed evaluator, whatever the number of units
    const bool big = P.big != 0 && !wide1;
    if (big) solo = wave = false;
    pl.wave = !wave ? WaveUse::never : ((env.wave == 1 || !solo_cap) ? WaveUse::always : WaveUse::by_live);
    if (wave) pl.geomw = wave_geometry(P.nf, P.blk[0].K, P.D, P.nblocks);

    // the 16-chain kernel's LDS is the limit whatever starts the run (the one-chain kernels of a later hand-over live within it)
    plan_tile16(pl, P, env);
    // chains per workgroup: fill every CU with one workgroup before putting a second chain on any wave
    pl.cpw = std::min(NC, std::max(1, forced_cpw ? env.cpw : (n_units + n_cu - 1) / n_cu));
    pl.n_wg = (n_units + pl.cpw - 1) / pl.cpw;
    pl.may_migrate = may_migrate;
    if (wide1 || big) plan_wide(pl, P, n_units, big, row_stride(P.D), WIDE1_LDS_CAP);
    if (wide1) pl.lds_bytes = std::max(pl.lds_bytes, wide1_lds_bytes(pl.geom1, row_stride(P.D), pl.nhot));     // (one attribute value for every kernel)
    if (big) pl.lds_bytes = nuts_big_lds_bytes(big_njx(P.D));
    int rc = pl.lds_bytes > LDS_BUDGET ? 1 : 0;
    if (!rc && P.D > (big ? BIG_MAX_D : 32 * 27)) rc = 2;
    if (solo) plan_solo(pl, P, n_units, n_cu, env);
    // more workgroups than CUs: finished chains can be squeezed out of the tiles (BDRT_COMPACTION=0 keeps the layout)
    pl.may_compact = pl.layout == Layout::tile16 && pl.n_wg > n_cu && env.compaction != 0;
    return rc;
}

struct Sampler {
    Problem *prob = nullptr;
    NutsParams np;
    NutsArgs args;                    // what the kernels get: plain views of the buffers below
    SamplerPlan plan;                 // which kernel advances the run, and with what
    SamplerEnv env;
    int n_units = 0, D = 0, n_cu = 256;
    std::vector<int> spec;            // host copy: the spectrum of each unit (bdrt_sampler_loo: the data row of a group)
    Kernel last_one_chain = Kernel::solo;   // the kernel of the last launch in the solo layout (bdrt_sampler_kind)
    int live = 0;                     // chains of the solo layout still running (after the last launch that read the done counter)
    hipStream_t stream = nullptr;
    double ms_total = 0.0; int64_t n_launch = 0;     // kernel time and launches (bdrt_sampler_kernel_time)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    int rounds_default = 256;
    DevBuf<double> vecs, draws, lp_draws, bigws;
    DevBuf<ChainState> states;
    DevBuf<int> d_done, d_active;     // finished workgroups / live chains of the 16-chain kernel after the last launch
    DevBuf<unsigned long long> d_leaps;
    DevBuf<long long> d_prof;
    int prof_wg = 0;                  // workgroups d_prof was allocated for (the layout can change under it: compaction, tail migration)
    // tail migration: the 16-chain rows, kept until the sampler is destroyed, and unit of workgroup b of the one-chain kernel
    DevBuf<double> vecs16;
    DevBuf<int> d_unit_map;
    bool migrated() const { return d_unit_map != nullptr; }
    // unit <-> slot of the 16-chain kernel (compaction: nuts_compact_kernel)
    std::vector<int> slot_unit;       // host copy of args.slot_unit: [n_wg][16]
    std::vector<int> unit_loc;        // unit -> wg * 16 + slot (-1: retired: the chain had finished when its workgroup was re-packed)
    DevBuf<int> d_slot_unit, d_unit_loc;
    size_t vecs_capacity = 0;         // doubles allocated behind args.vecs
    DevBuf<double> vecs_alt;          // second buffer of the same size: re-packing ping-pongs between the two (no allocation,
    DevBuf<int> d_slot_alt, d_live;   //  hence no implicit device synchronisation, per pass)
    int n_compactions = 0;
};

// an integer environment variable (`unset` when it is not there); as a flag: -1 not there, else 0 / 1
static int env_int(const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; }
static int env_flag(const char *name) { const int v = env_int(name, INT_MIN); return v == INT_MIN ? -1 : (v != 0 ? 1 : 0); }
static SamplerEnv read_sampler_env()
{
    SamplerEnv env;
    env.solo = env_flag("BDRT_SOLO"); env.wave = env_flag("BDRT_WAVE"); env.wide1 = env_flag("BDRT_WIDE1");
    env.tail_migration = env_flag("BDRT_TAIL_MIGRATION"); env.compaction = env_flag("BDRT_COMPACTION"); env.solo_duo = env_flag("BDRT_SOLO_DUO");
    env.cpw = env_int("BDRT_CHAINS_PER_WG", INT_MIN); env.s1_ku6 = env_int("BDRT_S1_KU", 0) == 6;
    return env;
}

}  // namespace bdrt

using namespace bdrt;

struct bdrt_sampler {
    bdrt::Sampler impl;
};

extern "C" {

void bdrt_nuts_defaults(bdrt_nuts_control *c)
{
    c->adapt_delta = 0.9; c->adapt_t0 = 10; c->adapt_gamma = 0.05; c->adapt_kappa = 0.75;
    c->max_treedepth = 10; c->init_buffer = 75; c->term_buffer = 50; c->base_window = 25;
    c->init_radius = 2; c->max_deltaH = 1000; c->stepsize0 = 1;
}

void bdrt_sampler_destroy(bdrt_sampler *s)
{
    if (!s) return;
    Sampler &S = s->impl;
    if (S.stream) hipStreamSynchronize(S.stream);
    for (auto &pr : S.pending) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
    if (S.stream) hipStreamDestroy(S.stream);
    delete s;
}

bdrt_sampler *bdrt_sampler_create(bdrt_problem *p, int n_units, const int *spec, const int *chain_id, int warmup,
                                  int n_draws, uint64_t seed, const double *init_theta, const bdrt_nuts_control *ctrl)
{
    if (!p || n_units < 1 || warmup < 0 || n_draws < 0) { set_error("bdrt_sampler_create: bad arguments"); return nullptr; }
    bdrt_nuts_control c;
    if (ctrl) c = *ctrl; else bdrt_nuts_defaults(&c);
    if (c.max_treedepth < 1 || c.max_treedepth > MAXD) { set_error("max_treedepth must be in [1,%d]", MAXD); return nullptr; }
    // Stan's argument checks (stan::services: adapt delta in (0,1), gamma / kappa / t0 / stepsize > 0, init radius >= 0); written so
    // that NaN fails them.  Nonsense here does not crash a kernel, it silently gives nonsense chains.
    if (!(c.adapt_delta > 0.0 && c.adapt_delta < 1.0)) { set_error("bdrt_sampler_create: adapt_delta must be in (0,1)"); return nullptr; }
    if (!(c.adapt_gamma > 0.0) || !(c.adapt_kappa > 0.0) || !(c.adapt_t0 > 0.0)) { set_error("bdrt_sampler_create: adapt_gamma, adapt_kappa, adapt_t0 must be positive"); return nullptr; }
    if (!(c.stepsize0 > 0.0) || !std::isfinite(c.stepsize0)) { set_error("bdrt_sampler_create: stepsize0 must be positive and finite"); return nullptr; }
    if (!(c.init_radius >= 0.0) || !std::isfinite(c.init_radius)) { set_error("bdrt_sampler_create: init_radius must be >= 0 and finite"); return nullptr; }
    if (!(c.max_deltaH > 0.0)) { set_error("bdrt_sampler_create: max_deltaH must be positive"); return nullptr; }
    if (c.init_buffer < 0 || c.term_buffer < 0 || c.base_window < 0) { set_error("bdrt_sampler_create: adaptation window sizes must be >= 0"); return nullptr; }
    Problem &P = p->impl;
    if (hipSetDevice(P.device) != hipSuccess) { set_error("bdrt_sampler_create: hipSetDevice(%d) failed", P.device); return nullptr; }
    bdrt_sampler *s = new bdrt_sampler();
    Sampler &S = s->impl;
    auto fail = [&](const char *fmt, auto... a) -> bdrt_sampler * { set_error(fmt, a...); bdrt_sampler_destroy(s); return nullptr; };
    memset(&S.args, 0, sizeof(S.args));
    S.prob = &P; S.n_units = n_units; S.D = P.dev.D;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, P.device) == hipSuccess && prop.multiProcessorCount > 0) S.n_cu = prop.multiProcessorCount;
    S.env = read_sampler_env();
    const int plan_rc = make_plan(P.dev, n_units, S.n_cu, S.env, S.plan);
    const SamplerPlan &pl = S.plan;
    S.np.warmup = warmup; S.np.n_draws = n_draws; S.np.max_depth = c.max_treedepth;
    S.np.delta = c.adapt_delta; S.np.gamma = c.adapt_gamma; S.np.t0 = c.adapt_t0; S.np.kappa = c.adapt_kappa;
    S.np.init_radius = c.init_radius; S.np.max_deltaH = c.max_deltaH; S.np.stepsize0 = c.stepsize0;
    S.np.seed_lo = (uint32_t)seed; S.np.seed_hi = (uint32_t)(seed >> 32);
    S.np.has_init = init_theta != nullptr;
    if (plan_rc == 1) return fail("bdrt_sampler_create: problem too large for the 160 KiB LDS budget");
    for (int u = 0; u < n_units; ++u)
        if (spec && (spec[u] < 0 || spec[u] >= P.dev.n_spectra)) return fail("bdrt_sampler_create: spectrum index out of range");
    if (plan_rc == 2) return fail("bdrt_sampler_create: D = %d > %d not supported", S.D, pl.kernel == Kernel::big ? BIG_MAX_D : 864);

    // the state rows, filled on the host: [n_wg][nrow][ncol][ds]
    const bool tiles = pl.layout == Layout::tile16, solo_rows = pl.layout == Layout::solo;
    const int DS = pl.ds;
    S.args.cpw = pl.cpw; S.args.ds = DS;
    const int ncol = tiles ? NC : 1, nrow = solo_rows ? (int)SG_COUNT : (int)V_COUNT;
    const int r_minv = solo_rows ? (int)SV_MINV : (int)V_MINV, r_th = solo_rows ? (int)SV_TH : (int)V_TH;
    const size_t nvec = (size_t)pl.n_wg * nrow * ncol * DS;
    std::vector<double> hv(nvec, 0.0);
    std::vector<ChainState> hs((size_t)n_units);
    for (int u = 0; u < n_units; ++u) {
        ChainState &st = hs[u];
        memset(&st, 0, sizeof(st));
        st.phase = PH_INIT;
        st.z_iter = -1;
        st.spec = spec ? spec[u] : 0;
        S.spec.push_back(st.spec);
        st.chain_id = chain_id ? chain_id[u] : u;
        st.eps = c.stepsize0;
        st.dir = 1;
        st.lsw_sub = -INFINITY;
        window_init(st, warmup, c.init_buffer, c.term_buffer, c.base_window);
        const int wg = u / pl.cpw, cc = tiles ? slot_col(u % pl.cpw) : 0;
        double *V = hv.data() + (size_t)wg * nrow * ncol * DS;
        const Philox rng = {S.np.seed_lo, S.np.seed_hi, (uint32_t)st.chain_id};
        for (int j = 0; j < S.D; ++j) {
            V[((size_t)r_minv * ncol + cc) * DS + j] = 1.0;
            V[((size_t)r_th * ncol + cc) * DS + j] =
                init_theta ? init_theta[(size_t)u * S.D + j]
                           : c.init_radius * (2.0 * rng_uniform(rng, (uint32_t)j, RNG_INIT, 0, 0, 0) - 1.0);
        }
        if (!init_theta) st.init_attempt = 0;
    }
    // unused columns (cpw < 16, last workgroup): finite placeholders
    for (int wg = 0; wg < pl.n_wg && tiles; ++wg)
        for (int k = 0; k < NC; ++k) {
            if (k < pl.cpw && wg * pl.cpw + k < n_units) continue;
            double *V = hv.data() + (size_t)wg * V_COUNT * NC * DS;
            for (int j = 0; j < S.D; ++j) V[((size_t)V_MINV * NC + slot_col(k)) * DS + j] = 1.0;
        }
    if (tiles) {
        S.slot_unit.assign((size_t)pl.n_wg * NC, -1);
        S.unit_loc.assign((size_t)n_units, -1);
        for (int u = 0; u < n_units; ++u) {
            const int wg = u / pl.cpw, k = u % pl.cpw;
            S.slot_unit[(size_t)wg * NC + k] = u;
            S.unit_loc[u] = wg * NC + k;
        }
        if (S.d_slot_unit.alloc(S.slot_unit.size()) != hipSuccess || S.d_unit_loc.alloc(S.unit_loc.size()) != hipSuccess)
            return fail("hipMalloc(slot map) failed");
        if (hipMemcpy(S.d_slot_unit, S.slot_unit.data(), S.slot_unit.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(S.d_unit_loc, S.unit_loc.data(), S.unit_loc.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess)
            return fail("bdrt_sampler_create: upload of the slot map failed");
        S.args.slot_unit = S.d_slot_unit;
    }
    S.vecs_capacity = nvec;
    const size_t nlp = (size_t)n_units * std::max(n_draws, 1), nd = nlp * S.D;
    if (S.vecs.alloc(nvec) != hipSuccess) return fail("hipMalloc(vecs) failed");
    if (S.states.alloc(hs.size()) != hipSuccess) return fail("hipMalloc(states) failed");
    if (S.draws.alloc(nd) != hipSuccess) return fail("hipMalloc(draws) failed");
    if (S.lp_draws.alloc(nlp) != hipSuccess) return fail("hipMalloc(lp) failed");
    if (S.d_done.alloc(1) != hipSuccess || S.d_leaps.alloc(1) != hipSuccess || S.d_active.alloc(1) != hipSuccess) return fail("hipMalloc failed");
    if (pl.kernel == Kernel::big && S.bigws.alloc((size_t)pl.n_wg * big_ws_doubles(P.dev)) != hipSuccess) return fail("hipMalloc(workspace) failed");
    if (hipMemcpy(S.vecs, hv.data(), nvec * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return fail("bdrt_sampler_create: upload of the chain vectors failed");
    if (hipMemcpy(S.states, hs.data(), hs.size() * sizeof(ChainState), hipMemcpyHostToDevice) != hipSuccess)
        return fail("bdrt_sampler_create: upload of the chain states failed");
    if (hipMemset(S.draws, 0, nd * sizeof(double)) != hipSuccess) return fail("bdrt_sampler_create: clearing the draws failed");
    if (hipMemset(S.d_leaps, 0, sizeof(unsigned long long)) != hipSuccess)
        return fail("bdrt_sampler_create: clearing the leapfrog counter failed");
    // hipMemset returns before the fill has happened, and the sampler's kernels run on a NON-BLOCKING stream that does not order
    // itself behind the null stream: without this wait a launch that follows quickly (several host threads sampling at once)
    // can have its first draws / its leapfrog counter zeroed under it.
    if (hipStreamSynchronize(nullptr) != hipSuccess) return fail("bdrt_sampler_create: initial fills failed");
    S.args.vecs = S.vecs; S.args.states = S.states; S.args.draws = S.draws; S.args.lp_draws = S.lp_draws;
    S.args.bigws = S.bigws; S.args.leap_counter = S.d_leaps; S.args.done_counter = S.d_done; S.args.active_counter = S.d_active;
    S.args.n_units = S.live = n_units;
    if (hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking) != hipSuccess) return fail("hipStreamCreate failed");
    const hipError_t ae = nuts_set_lds_limit(pl.lds_bytes);
    if (ae != hipSuccess) return fail("hipFuncSetAttribute(nuts_kernel, %zu B dynamic LDS) failed: %s", pl.lds_bytes, hipGetErrorString(ae));
    return s;
}

static int harvest_events(Sampler &S, bool wait)
{
    size_t k = 0;
    for (; k < S.pending.size(); ++k) {
        auto &pr = S.pending[k];
        if (!wait && hipEventQuery(pr.second) != hipSuccess) break;
        if (wait) BDRT_HIP(hipEventSynchronize(pr.second));
        float ms = 0.f;
        BDRT_HIP(hipEventElapsedTime(&ms, pr.first, pr.second));
        S.ms_total += ms;
        hipEventDestroy(pr.first); hipEventDestroy(pr.second);
    }
    S.pending.erase(S.pending.begin(), S.pending.begin() + k);
    return 0;
}

// one launch of the plan's kernel
static int launch_plan(Sampler &S)
{
    const SamplerPlan &pl = S.plan;
    const DevProblem *dp = (const DevProblem *)S.prob->d_dev;
    const Kernel kernel = kernel_for_launch(pl, S.live, S.n_cu);
    if (pl.layout == Layout::solo) S.last_one_chain = kernel;
    if (kernel == Kernel::wave) {
        // LDS share (= chains per CU) by the chains still running: finished ones leave their wave at once
        int nhot = 0;
        const size_t lds = wave_lds_request(pl.geomw, std::max(1, std::min(S.live, pl.n_wg)), S.n_cu, &nhot, wave_chains_per_cu(S.prob->dev));
        return launch_wave_nuts(dp, S.np, S.args, pl.geomw, nhot, pl.n_wg, lds, S.stream, S.prob->dev.outlier_mode != 0) ? -10 : 0;
    }
    if (kernel == Kernel::solo)
        return launch_nuts(pl.key, dp, S.np, S.args, pl.n_wg, pl.key.a == 4 ? solo_duo_lds_bytes(pl.geom) : pl.lds_bytes, S.stream, &pl.geom);
    if (kernel == Kernel::wide1)
        return launch_nuts(pl.key, dp, S.np, S.args, pl.n_wg, wide1_lds_bytes(pl.geom1, S.args.ds, pl.nhot), S.stream, &pl.geom1, &pl.nhot);
    return launch_nuts(pl.key, dp, S.np, S.args, pl.n_wg, pl.lds_bytes, S.stream);       // (tile16, big)
}

int bdrt_sampler_advance(bdrt_sampler *s, int rounds, int *all_done)
{
    if (!s || rounds < 1) { set_error("bdrt_sampler_advance: bad arguments"); return -1; }
    Sampler &S = s->impl;
    BDRT_HIP(hipSetDevice(S.prob->device));
    S.args.rounds = rounds;
    BDRT_HIP(hipMemsetAsync(S.d_done, 0, sizeof(int), S.stream));
    BDRT_HIP(hipMemsetAsync(S.d_active, 0, sizeof(int), S.stream));
    hipEvent_t e0, e1;
    BDRT_HIP(hipEventCreate(&e0));
    BDRT_HIP(hipEventCreate(&e1));
    BDRT_HIP(hipEventRecord(e0, S.stream));
    if (const int rc = launch_plan(S)) { hipEventDestroy(e0); hipEventDestroy(e1); return rc; }
    BDRT_HIP(hipEventRecord(e1, S.stream));
    S.pending.emplace_back(e0, e1);
    S.n_launch += 1;
    if (all_done) {
        int done = 0;
        BDRT_HIP(hipMemcpyAsync(&done, S.d_done, sizeof(int), hipMemcpyDeviceToHost, S.stream));
        BDRT_HIP(hipStreamSynchronize(S.stream));
        *all_done = done >= S.plan.n_wg;
        if (S.plan.layout == Layout::solo) S.live = std::max(0, S.plan.n_wg - done);
        return harvest_events(S, true);
    }
    return harvest_events(S, false);
}

int bdrt_sampler_sync(bdrt_sampler *s)
{
    if (!s) return -1;
    Sampler &S = s->impl;
    BDRT_HIP(hipStreamSynchronize(S.stream));
    // the live-chain count that picks the next launch's kernel (one chain per wave / per workgroup, the wave kernel's LDS share):
    // `advance(..., NULL)` does not read the launch's done counter back, a sync does (the last launch wrote it)
    if (S.plan.layout == Layout::solo && S.n_launch > 0) {
        int done = 0;
        BDRT_HIP(hipMemcpy(&done, S.d_done, sizeof(int), hipMemcpyDeviceToHost));
        S.live = std::max(0, S.plan.n_wg - done);
    }
    return harvest_events(S, true);
}

// Re-pack the live chains of a 16-chain run into fewer workgroups (nuts_compact_kernel).  Called between launches with the
// stream idle and `active` = live chains after the last launch.  Worth it only while the run has more workgroups than CUs:
// with one workgroup per CU a round costs the same whatever the number of live columns, and fewer workgroups would only idle CUs.
static int maybe_compact(Sampler &S, int active)
{
    if (!S.plan.may_compact || S.plan.layout != Layout::tile16 || active <= 0) return 0;
    const int target = std::max(S.n_cu, (active + NC - 1) / NC);
    // A launch runs its workgroups in turns of one per CU, and every turn lasts the full `rounds` however many CUs it fills:
    // what a re-packing buys is a whole turn, so it is done when -- and only when -- the live chains fit in one turn less
    // (measured on 1536 spectra x 8 chains: re-packing at every 1/16 of the workgroups, 15 passes, 32.7 s; at the turn
    // boundaries 8192 and 4096 live chains ... see profiles/r03/oversubscribed.txt; frozen layout 36.6 s)
    if ((target + S.n_cu - 1) / S.n_cu >= (S.plan.n_wg + S.n_cu - 1) / S.n_cu) return 0;
    if (!S.vecs_alt) {
        // the second buffer and the liveness flags, once (keep going as is when the memory is not there)
        if (S.vecs_alt.alloc(S.vecs_capacity) != hipSuccess || S.d_slot_alt.alloc(S.slot_unit.size()) != hipSuccess ||
            S.d_live.alloc((size_t)S.n_units) != hipSuccess) { (void)hipGetLastError(); S.plan.may_compact = false; return 0; }
    }
    std::vector<int> alive((size_t)S.n_units);
    if (const int rc = launch_nuts_live(S.states, S.n_units, S.d_live, S.stream)) return rc;
    BDRT_HIP(hipMemcpyAsync(alive.data(), S.d_live, alive.size() * sizeof(int), hipMemcpyDeviceToHost, S.stream));
    BDRT_HIP(hipStreamSynchronize(S.stream));
    std::vector<int> live;
    for (int wgk = 0; wgk < (int)S.slot_unit.size(); ++wgk) {            // slot order: keeps neighbours (same spectrum) together
        const int u = S.slot_unit[wgk];
        if (u >= 0 && alive[u]) live.push_back(u);
    }
    if (live.empty()) return 0;
    const int n_wg = std::max(std::min(S.n_cu, (int)live.size()), ((int)live.size() + NC - 1) / NC);
    const int cpw = ((int)live.size() + n_wg - 1) / n_wg;
    std::vector<int> slot_unit((size_t)n_wg * NC, -1), unit_loc((size_t)S.n_units, -1);
    for (size_t i = 0; i < live.size(); ++i) {
        const int wg = (int)(i / cpw), k = (int)(i % cpw);
        slot_unit[(size_t)wg * NC + k] = live[i];
        unit_loc[live[i]] = wg * NC + k;
    }
    BDRT_HIP(hipMemcpyAsync(S.d_slot_alt, slot_unit.data(), slot_unit.size() * sizeof(int), hipMemcpyHostToDevice, S.stream));
    // d_unit_loc still holds the OLD locations: the kernel reads them, then they are replaced
    if (const int rc = launch_nuts_compact(S.vecs, S.d_unit_loc, S.d_slot_alt, n_wg, S.vecs_alt, S.args.ds, S.stream)) return rc;
    BDRT_HIP(hipMemcpyAsync(S.d_unit_loc, unit_loc.data(), unit_loc.size() * sizeof(int), hipMemcpyHostToDevice, S.stream));
    BDRT_HIP(hipStreamSynchronize(S.stream));            // (the host vectors above are read by the asynchronous copies)
    std::swap(S.vecs, S.vecs_alt);
    std::swap(S.d_slot_unit, S.d_slot_alt);
    S.args.vecs = S.vecs;
    S.args.slot_unit = S.d_slot_unit;
    S.slot_unit.swap(slot_unit);
    S.unit_loc.swap(unit_loc);
    S.plan.n_wg = n_wg;
    S.n_compactions += 1;
    S.args.prof = nullptr;                               // (the phase-profile slots were laid out for the old workgroups)
    return 0;
}

// The tail of a large run.  The 16-chain kernel advances every live chain by one leapfrog per ~33 us whatever the number of live
// chains, a run lasts as long as its longest chain (BASELINE config 4: 0.33 .. 0.98 M leapfrogs per chain), and in the tail most
// tile columns are empty: the live chains go to a one-chain kernel when that finishes them sooner, and the tail's plan replaces the
// run's.  Called between launches with the stream idle.
static int maybe_migrate_tail(Sampler &S, int active)
{
    const DevProblem &P = S.prob->dev;
    const SamplerPlan &cur = S.plan;
    // the one-chain kernels run one or two chains per CU at a time, ~4x faster per leapfrog: the LDS-resident one wins below ~4.75
    // live chains per CU when two of its workgroups fit a CU (else ~3.5), the general one below ~2.75
    // (the one-chain-per-wave kernel runs eight chains per CU at 108 M evals/s against 73 M of half-empty tiles: profiles/r04/wave_sweep.txt)
    const bool by_wave = cur.wave != WaveUse::never, to_solo = solo_capable(P) || by_wave;
    const int limit = by_wave ? wave_max_units(S.n_cu, P) : (to_solo ? (solo_duo_fits(P, S.env) ? (19 * S.n_cu) / 4 : (7 * S.n_cu) / 2) : (11 * S.n_cu) / 4);
    if (active <= 0 || active > limit) return 0;
    std::vector<ChainState> hs((size_t)S.n_units);
    BDRT_HIP(hipMemcpy(hs.data(), S.states, hs.size() * sizeof(ChainState), hipMemcpyDeviceToHost));
    std::vector<int> map;
    for (int u = 0; u < S.n_units; ++u)
        if (chain_running(hs[u].phase)) map.push_back(u);
    if (map.empty()) return 0;
    SamplerPlan tail = cur;
    if (to_solo) {
        plan_solo(tail, P, (int)map.size(), S.n_cu, S.env);
        if (solo_capable(P) && tail.lds_bytes > cur.lds_bytes) return 0;     // (bdrt_sampler_create raised every kernel's LDS limit to the 16-chain size)
    } else {
        // general one-chain kernel: the 16-chain rows, one column; as many LDS-resident rows as the LDS limit set at creation allows
        plan_wide(tail, P, (int)map.size(), false, cur.ds, std::min(cur.lds_bytes, WIDE1_LDS_CAP));
        if (wide1_lds_bytes(tail.geom1, cur.ds, tail.nhot) > cur.lds_bytes) return 0;
    }
    DevBuf<double> vnew;
    DevBuf<int> dmap;
    const size_t rows = to_solo ? (size_t)SG_COUNT * tail.ds : (size_t)V_COUNT * cur.ds;
    if (vnew.alloc(map.size() * rows) != hipSuccess || dmap.alloc(map.size()) != hipSuccess) { (void)hipGetLastError(); return 0; }   // (keep going as is)
    BDRT_HIP(hipMemcpy(dmap, map.data(), map.size() * sizeof(int), hipMemcpyHostToDevice));
    if (const int rc = launch_nuts_migrate(to_solo, S.vecs, cur.ds, S.d_unit_loc, dmap, tail.n_wg, vnew, tail.ds, S.D, S.states, S.stream)) return rc;
    BDRT_HIP(hipStreamSynchronize(S.stream));
    S.vecs16 = std::move(S.vecs);
    S.vecs = std::move(vnew);
    S.d_unit_map = std::move(dmap);
    S.args.vecs = S.vecs;
    S.args.unit_map = S.d_unit_map;
    S.args.ds = tail.ds;
    S.args.prof = nullptr;                                // (the phase-profile slots are laid out per 16-chain workgroup)
    S.live = tail.n_wg;
    S.plan = tail;                                        // (n_wg = the chains handed over: the all-done test counts finished workgroups)
    return 0;
}

int bdrt_sampler_run(bdrt_sampler *s)
{
    if (!s) return -1;
    Sampler &S = s->impl;
    // upper bound on the leapfrogs one chain can need: (2^depth - 1 + step-size trials) per iteration
    const long long per_iter = (1LL << S.np.max_depth) + 64;
    const long long bound = per_iter * (S.np.warmup + S.np.n_draws + 2) + 200;
    long long spent = 0;
    int done = 0;
    while (!done && spent <= bound) {
        int rc = bdrt_sampler_advance(s, S.rounds_default, &done);
        if (rc) return rc;
        spent += S.rounds_default;
        if (!done && !S.migrated() && (S.plan.may_migrate || S.plan.may_compact)) {
            int active = 0;
            BDRT_HIP(hipMemcpy(&active, S.d_active, sizeof(int), hipMemcpyDeviceToHost));
            if (S.plan.may_migrate && (rc = maybe_migrate_tail(S, active))) return rc;
            if (!S.migrated() && (rc = maybe_compact(S, active))) return rc;
        }
    }
    if (!done) { set_error("bdrt_sampler_run: chains did not finish within the leapfrog bound"); return -3; }
    return 0;
}

int bdrt_sampler_results(bdrt_sampler *s, double *draws, double *lp, bdrt_chain_diag *diag)
{
    if (!s) return -1;
    Sampler &S = s->impl;
    BDRT_HIP(hipStreamSynchronize(S.stream));
    const size_t nd = (size_t)S.n_units * S.np.n_draws;
    if (draws && nd) BDRT_HIP(hipMemcpy(draws, S.args.draws, nd * S.D * sizeof(double), hipMemcpyDeviceToHost));
    if (lp && nd) BDRT_HIP(hipMemcpy(lp, S.args.lp_draws, nd * sizeof(double), hipMemcpyDeviceToHost));
    if (diag) {
        std::vector<ChainState> hs((size_t)S.n_units);
        BDRT_HIP(hipMemcpy(hs.data(), S.args.states, hs.size() * sizeof(ChainState), hipMemcpyDeviceToHost));
        for (int u = 0; u < S.n_units; ++u) {
            diag[u].n_leapfrog = hs[u].n_leap_total;
            diag[u].n_divergent = hs[u].n_div;
            diag[u].n_max_treedepth = hs[u].n_maxdepth;
            diag[u].stepsize = hs[u].eps;
            diag[u].mean_accept = hs[u].n_post ? hs[u].sum_accept / hs[u].n_post : 0.0;
            if (hs[u].phase == PH_FAILED) diag[u].n_leapfrog = -1;
        }
    }
    return 0;
}

int bdrt_sampler_tail_units(bdrt_sampler *s) { return s && s->impl.migrated() ? s->impl.plan.n_wg : 0; }
int bdrt_sampler_compactions(bdrt_sampler *s) { return s ? s->impl.n_compactions : -1; }
int bdrt_sampler_kind(bdrt_sampler *s)
{
    if (!s) return -1;
    const Sampler &S = s->impl;
    if (S.plan.layout != Layout::solo) return (int)S.plan.kernel;
    // before the first launch: what the first launch will use
    return (int)(S.n_launch ? S.last_one_chain : kernel_for_launch(S.plan, S.live, S.n_cu));
}

int64_t bdrt_sampler_total_leapfrogs(bdrt_sampler *s)
{
    if (!s) return -1;
    Sampler &S = s->impl;
    unsigned long long v = 0;
    if (hipStreamSynchronize(S.stream) != hipSuccess) return -1;
    if (hipMemcpy(&v, S.d_leaps, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int64_t)v;
}

int bdrt_sampler_kernel_time(bdrt_sampler *s, double *ms_total, int64_t *n_launches, int reset)
{
    if (!s) return -1;
    Sampler &S = s->impl;
    BDRT_HIP(hipStreamSynchronize(S.stream));
    int rc = harvest_events(S, true);
    if (rc) return rc;
    if (ms_total) *ms_total = S.ms_total;
    if (n_launches) *n_launches = S.n_launch;
    if (reset) { S.ms_total = 0.0; S.n_launch = 0; }
    return 0;
}

int bdrt_sampler_phase_profile(bdrt_sampler *s, int enable, long long *cycles32)
{
    if (!s) return -1;
    Sampler &S = s->impl;
    BDRT_HIP(hipStreamSynchronize(S.stream));
    // d_prof holds prof_wg workgroups' slots: the layout may have changed since (compaction, tail migration switch the profile off
    // and can leave MORE workgroups than it was allocated for) -- every copy / fill below is sized by the allocation
    if (cycles32) {
        for (int k = 0; k < 32; ++k) cycles32[k] = 0;
        if (S.d_prof) {
            std::vector<long long> h((size_t)S.prof_wg * 32);
            BDRT_HIP(hipMemcpy(h.data(), S.d_prof, h.size() * sizeof(long long), hipMemcpyDeviceToHost));
            for (int w = 0; w < S.prof_wg; ++w)
                for (int k = 0; k < 32; ++k) cycles32[k] += h[(size_t)w * 32 + k];
        }
    }
    if (S.d_prof && (!enable || S.prof_wg < S.plan.n_wg)) { S.d_prof.reset(); S.prof_wg = 0; }
    if (enable && !S.d_prof) {
        BDRT_HIP(S.d_prof.alloc((size_t)S.plan.n_wg * 32));
        S.prof_wg = S.plan.n_wg;
    }
    if (S.d_prof) {
        BDRT_HIP(hipMemset(S.d_prof, 0, (size_t)S.prof_wg * 32 * sizeof(long long)));
        BDRT_HIP(hipStreamSynchronize(nullptr));        // (same ordering rule as in bdrt_sampler_create)
    }
    S.args.prof = S.d_prof;
    return 0;
}

// Common front of the reductions over a sampler's draws: units [unit_lo, unit_hi) must exist, hold draws and, with
// chains_per_group > 0, split into groups of that many chains.  Binds the calling thread to the sampler's device, waits for the
// sampler's stream and gives the first draw of unit_lo in *dX.  who: the caller's name and its word for the range, which open
// the message ("bdrt_sampler_summary: bad unit" range).
static int sampler_draws(const char *who, bdrt_sampler *s, int unit_lo, int unit_hi, int chains_per_group, const double **dX)
{
    Sampler &S = s->impl;
    if (unit_lo < 0 || unit_hi > S.n_units || unit_lo >= unit_hi || (chains_per_group && (unit_hi - unit_lo) % chains_per_group) ||
        S.np.n_draws < 1) {
        set_error("%s range", who);
        return -1;
    }
    BDRT_HIP(hipSetDevice(S.prob->device));
    BDRT_HIP(hipStreamSynchronize(S.stream));
    *dX = S.args.draws + (size_t)unit_lo * S.np.n_draws * S.D;
    return 0;
}

int bdrt_sampler_percentiles(bdrt_sampler *s, int unit_lo, int unit_hi, int col0, int ncols, const double *Phi, int M,
                             const double *bias, const double *q, int nq, double *out)
{
    if (!s || !q || nq < 1 || !out) { set_error("bdrt_sampler_percentiles: null argument"); return -1; }
    Sampler &S = s->impl;
    if (col0 < 0 || ncols < 1 || col0 + ncols > S.D || (Phi && M < 1)) {
        set_error("bdrt_sampler_percentiles: bad unit / column range");
        return -1;
    }
    const double *dX;
    if (int rc = sampler_draws("bdrt_sampler_percentiles: bad unit / column", s, unit_lo, unit_hi, 0, &dX)) return rc;
    const long rows = (long)(unit_hi - unit_lo) * S.np.n_draws;
    if (rows > (1L << 30)) { set_error("bdrt_sampler_percentiles: too many rows"); return -1; }
    return post_percentiles_device(dX + col0, (int)rows, ncols, (long)S.D, Phi, M, bias, q, nq, out);
}

int bdrt_sampler_summary(bdrt_sampler *s, int unit_lo, int unit_hi, const double *q, int nq, double *mean, double *pct)
{
    if (!s || !q || nq < 1 || !pct) { set_error("bdrt_sampler_summary: null argument"); return -1; }
    Sampler &S = s->impl;
    const double *dX;
    if (int rc = sampler_draws("bdrt_sampler_summary: bad unit", s, unit_lo, unit_hi, 0, &dX)) return rc;
    const long rows = (long)(unit_hi - unit_lo) * S.np.n_draws;
    if (rows > (1L << 30)) { set_error("bdrt_sampler_summary: too many rows"); return -1; }
    return post_percentiles_device(dX, (int)rows, S.D, (long)S.D, nullptr, 0, nullptr, q, nq, pct, S.prob->is_pos.data(), mean);
}

int bdrt_sampler_diagnostics(bdrt_sampler *s, int unit_lo, int unit_hi, int chains_per_group, double *mean, double *sd,
                             double *n_eff, double *rhat)
{
    if (!s || chains_per_group < 1) { set_error("bdrt_sampler_diagnostics: bad arguments"); return -1; }
    Sampler &S = s->impl;
    const double *dX;
    if (int rc = sampler_draws("bdrt_sampler_diagnostics: bad unit", s, unit_lo, unit_hi, chains_per_group, &dX)) return rc;
    return diagnostics_to_host(dX, (long)S.np.n_draws * S.D, (long)S.D, S.prob->is_pos.data(), (unit_hi - unit_lo) / chains_per_group,
                               chains_per_group, S.np.n_draws, S.D, mean, sd, n_eff, rhat, S.stream);
}

int bdrt_sampler_rank_diagnostics(bdrt_sampler *s, int unit_lo, int unit_hi, int chains_per_group, double p_lo, double p_hi,
                                  double *rhat, double *ess_bulk, double *ess_tail, double *ess_mean, double *sd)
{
    if (!s || chains_per_group < 1) { set_error("bdrt_sampler_rank_diagnostics: bad arguments"); return -1; }
    Sampler &S = s->impl;
    const double *dX;
    if (int rc = sampler_draws("bdrt_sampler_rank_diagnostics: bad unit", s, unit_lo, unit_hi, chains_per_group, &dX)) return rc;
    return rank_diagnostics_to_host(dX, (long)S.np.n_draws * S.D, (long)S.D, S.prob->is_pos.data(),
                                    (unit_hi - unit_lo) / chains_per_group, chains_per_group, S.np.n_draws, S.D, p_lo, p_hi, rhat,
                                    ess_bulk, ess_tail, ess_mean, sd, S.stream);
}

// Common front of bdrt_sampler_loo and bdrt_sampler_loo_predict: argument checks, sampler_draws, and the job for the device
// reductions (bdrt_host.h).  name: the entry point; spec: storage for the groups' spectra; n2: the scalar columns a group has
// (0: the 2 Nf of the problem's grid; bdrt_sampler_heldout: the 2 H of the held-out grid).
static int sampler_loo_job(const char *name, bdrt_sampler *s, int unit_lo, int unit_hi, int chains_per_group, int pair, int col0,
                           int ncols, int reff_mode, const double *reff_in, size_t chunk_bytes, std::vector<int> &spec, LooDraws &j,
                           int n2 = 0)
{
    if (!s || chains_per_group < 1 || (pair != 0 && pair != 1) || reff_mode < 0 || reff_mode > 2 || (reff_mode == 1 && !reff_in)) {
        set_error("%s: bad arguments", name);
        return -1;
    }
    Sampler &S = s->impl;
    const int N2 = n2 > 0 ? n2 : 2 * S.prob->dev.nf;
    if (col0 < 0 || ncols < 1 || col0 + ncols > N2 || (pair && (col0 != 0 || ncols != N2))) {
        set_error("%s: bad column range (pair = 1 needs all %d columns)", name, N2);
        return -1;
    }
    const std::string who = std::string(name) + ": bad unit";
    const double *dX;
    if (int rc = sampler_draws(who.c_str(), s, unit_lo, unit_hi, chains_per_group, &dX)) return rc;
    const long rows = (long)chains_per_group * S.np.n_draws;
    if (rows > bdrt_psis_loo_max_draws()) {
        set_error("%s: %ld draws per column, the kernel holds at most %d", name, rows, bdrt_psis_loo_max_draws());
        return -2;
    }
    if (rows < 2) { set_error("%s: at least 2 draws are needed", name); return -1; }
    const int G = (unit_hi - unit_lo) / chains_per_group;
    spec.resize((size_t)G);
    for (int g = 0; g < G; ++g) {
        const int u0 = unit_lo + g * chains_per_group;
        spec[g] = S.spec[u0];
        for (int m = 1; m < chains_per_group; ++m)
            if (S.spec[u0 + m] != spec[g]) { set_error("%s: the units of group %d were sampled against different spectra", name, g); return -1; }
    }
    j.prob = S.prob; j.draws = dX; j.spec = spec.data();
    j.G = G; j.chains = chains_per_group; j.n_draws = S.np.n_draws;
    j.pair = pair; j.col0 = col0; j.ncols = ncols;
    j.reff_mode = reff_mode; j.reff_in = reff_in; j.chunk_bytes = chunk_bytes; j.stream = S.stream;
    return 0;
}

int bdrt_sampler_loo(bdrt_sampler *s, int unit_lo, int unit_hi, int chains_per_group, int pair, int col0, int ncols, int reff_mode,
                     const double *reff_in, size_t chunk_bytes, double *lpd, double *elpd_loo, double *pareto_k, double *p_waic,
                     int *n_tail, double *reff_out)
{
    if (!lpd || !elpd_loo || !pareto_k || !p_waic || !n_tail) { set_error("bdrt_sampler_loo: null argument"); return -1; }
    std::vector<int> spec;
    LooDraws j;
    if (int rc = sampler_loo_job("bdrt_sampler_loo", s, unit_lo, unit_hi, chains_per_group, pair, col0, ncols, reff_mode, reff_in,
                                 chunk_bytes, spec, j))
        return rc;
    return loo_of_draws(j, lpd, elpd_loo, pareto_k, p_waic, n_tail, reff_out);
}

int bdrt_sampler_loo_predict(bdrt_sampler *s, int unit_lo, int unit_hi, int chains_per_group, int pair, int col0, int ncols,
                             int reff_mode, const double *reff_in, size_t chunk_bytes, double *mean, double *sd, double *pit,
                             double *mean_post, double *sd_post, double *pit_post, double *pareto_k, int *n_tail, double *reff_out)
{
    if (!mean || !sd || !pit || !mean_post || !sd_post || !pit_post || !pareto_k || !n_tail) {
        set_error("bdrt_sampler_loo_predict: null argument");
        return -1;
    }
    std::vector<int> spec;
    LooDraws j;
    if (int rc = sampler_loo_job("bdrt_sampler_loo_predict", s, unit_lo, unit_hi, chains_per_group, pair, col0, ncols, reff_mode,
                                 reff_in, chunk_bytes, spec, j))
        return rc;
    return loo_predict_of_draws(j, mean, sd, pit, mean_post, sd_post, pit_post, pareto_k, n_tail, reff_out);
}

int bdrt_sampler_heldout(bdrt_sampler *s, int unit_lo, int unit_hi, int chains_per_group, int pair, int col0, int ncols,
                         size_t chunk_bytes, const double *freq_test, int H, const double *A_test, const double *z_test, double *lpd,
                         double *mean, double *sd, double *pit)
{
    if (!freq_test || !A_test || !z_test || !lpd || !mean || !sd || !pit || H < 1) {
        set_error("bdrt_sampler_heldout: bad arguments");
        return -1;
    }
    if (s && s->impl.prob->dev.outlier_mode) {
        set_error("bdrt_sampler_heldout: outlier error models are refused: a held-out point has no sigma_out of its own");
        return -2;
    }
    if (heldout_check_grid("bdrt_sampler_heldout", freq_test, H)) return -1;
    std::vector<int> spec;
    LooDraws j;
    if (int rc = sampler_loo_job("bdrt_sampler_heldout", s, unit_lo, unit_hi, chains_per_group, pair, col0, ncols, 0, nullptr, chunk_bytes,
                                 spec, j, 2 * H))
        return rc;
    return heldout_of_draws(j, freq_test, H, A_test, z_test, lpd, mean, sd, pit);
}

int bdrt_sampler_heldout_mix(bdrt_sampler *s, int unit_lo, int unit_hi, int chains_per_group, int pair, int col0, int ncols,
                             size_t chunk_bytes, const double *freq_test, int H, const double *A_test, const double *z_test, int shared,
                             const double *y, const double *w, int Q, double ey2, double *lpd, double *mean, double *sd, double *pit)
{
    if (!freq_test || !A_test || !z_test || !y || !w || !lpd || !mean || !sd || !pit || H < 1) {
        set_error("bdrt_sampler_heldout_mix: bad arguments");
        return -1;
    }
    if (s && !s->impl.prob->dev.outlier_mode) {
        set_error("bdrt_sampler_heldout_mix: the problem has no outlier error model: bdrt_sampler_heldout is the entry for it");
        return -2;
    }
    if (heldout_check_grid("bdrt_sampler_heldout_mix", freq_test, H)) return -1;
    std::vector<int> spec;
    LooDraws j;
    if (int rc = sampler_loo_job("bdrt_sampler_heldout_mix", s, unit_lo, unit_hi, chains_per_group, pair, col0, ncols, 0, nullptr,
                                 chunk_bytes, spec, j, 2 * H))
        return rc;
    return heldout_mix_of_draws(j, freq_test, H, A_test, z_test, shared, y, w, Q, ey2, lpd, mean, sd, pit);
}

int bdrt_sampler_powerscale(bdrt_sampler *s, int unit_lo, int unit_hi, int chains_per_group, int col0, int ncols, double alpha_lo,
                            double alpha_hi, size_t chunk_bytes, double *cjs2, double *pareto_k, int *n_tail)
{
    const char *who = "bdrt_sampler_powerscale";
    if (!cjs2 || !pareto_k || !n_tail) { set_error("%s: null argument", who); return -1; }
    if (!(alpha_lo > 0.0) || !(alpha_lo < 1.0) || !(alpha_hi > 1.0) || !std::isfinite(alpha_hi)) {
        set_error("%s: the powers need 0 < alpha_lo < 1 < alpha_hi", who);
        return -1;
    }
    std::vector<int> spec;
    LooDraws j;
    if (int rc = sampler_loo_job(who, s, unit_lo, unit_hi, chains_per_group, 0, col0, ncols, 0, nullptr, chunk_bytes, spec, j)) return rc;
    const long rows = (long)chains_per_group * s->impl.np.n_draws;
    if (rows > bdrt_powerscale_max_draws()) {
        set_error("%s: %ld draws per column, the kernel holds at most %d", who, rows, bdrt_powerscale_max_draws());
        return -2;
    }
    return powerscale_of_draws(who, j, alpha_lo, alpha_hi, cjs2, pareto_k, n_tail, nullptr);
}

size_t bdrt_sampler_loo_group_bytes(bdrt_sampler *s, int chains_per_group, int pair, int ncols, int reff_mode, int predict)
{
    if (!s || chains_per_group < 1 || ncols < 1) return 0;
    LooDraws j = {};
    j.prob = s->impl.prob; j.chains = chains_per_group; j.n_draws = s->impl.np.n_draws;
    j.pair = pair; j.ncols = ncols; j.reff_mode = reff_mode;
    return loo_draws_group_bytes(j, predict != 0);
}

const double *bdrt_sampler_draws_dev(bdrt_sampler *s)
{
    if (!s) return nullptr;
    hipStreamSynchronize(s->impl.stream);
    return s->impl.args.draws;
}


int bdrt_sample(bdrt_problem *p, int n_units, const int *spec, const int *chain_id, int warmup, int n_draws,
                uint64_t seed, const double *init_theta, const bdrt_nuts_control *ctrl, double *draws, double *lp,
                bdrt_chain_diag *diag)
{
    bdrt_sampler *s = bdrt_sampler_create(p, n_units, spec, chain_id, warmup, n_draws, seed, init_theta, ctrl);
    if (!s) return -1;
    int rc = bdrt_sampler_run(s);
    if (rc == 0) rc = bdrt_sampler_results(s, draws, lp, diag);
    bdrt_sampler_destroy(s);
    return rc;
}

}  // extern "C"
