// Which kernels one sampler call runs: the ONE place that decides it.  Host-only, plain C++17, no HIP: a pure function of eight integers and
// the five A/B switches of the environment.  sd_kernels.hip builds a plan once per entry point and hands it down; sd_sampler_mode and
// sd_sampler_route report it.  Not part of the public ABI (the SD_ROUTE_* numbers are: include/soccerdiffusion_hip.h).
#ifndef SD_SAMPLER_PLAN_H
#define SD_SAMPLER_PLAN_H
#include <stdlib.h>
#include <string.h>

#include "../../include/soccerdiffusion_hip.h"

// Shapes the two trajectory families are instantiated for - pure shape predicates, each next to its instantiation table:
// tuned (sd_traj.hip): hidden_dim 256, 4 heads, horizon <= 100, 1 .. 64 memory rows, <= 32 joints, <= 8 layers;
// generic (sd_trajg.hip): hidden_dim 128 / 256 (horizon <= 100) or 512 (horizon <= 48), 4 heads, <= 8 layers, <= 32 joints, any memory length
bool traj_ok(int d, int heads, int T, int Mk, int J, int L);
bool trajg_ok(int d, int heads, int T, int Mk, int J, int L);

// the fused decoder-layer kernel applies: 4 heads == 4 waves each owning one head's columns (D >= 128), and at most 64 memory keys among
// the trajectories touching a 64-row panel
inline bool fused_layer_ok(int d, int heads, int T, int Mk) {
    if (heads != 4 || d < 128) return false;
    const int n_traj = (63 + T - 1) / T + 1;
    return (long)n_traj * Mk <= 64;
}

// The A/B switches, read once per process:
//   SD_SAMPLER_TRAJ=0    no trajectory kernels (the row-panel kernels of modes 0 - 2 instead)
//   SD_SAMPLER_GEMM=f32  no split-fp16 kernels at all: no trajectory kernels, no mode 2, no fp16 row chains
//   SD_SAMPLER_TRAJG=0   no generic trajectory kernels
//   SD_TRAJ_MAXROWS=n    memory rows beyond n go to the generic kernels instead of the tuned family's wide instantiation
//   SD_TRAJ_ROLLOUT=steps  no rollout kernel: every rollout on the tuned kernels is one launch per DDIM step
struct SamplerSwitches {
    bool traj, f16, trajg;
    int max_rows;
    bool rollout;
};
inline const SamplerSwitches &sampler_switches() {
    static const SamplerSwitches sw = [] {
        const auto is = [](const char *name, const char *value) {
            const char *e = getenv(name);
            return e && strcmp(e, value) == 0;
        };
        const char *mr = getenv("SD_TRAJ_MAXROWS");
        return SamplerSwitches{!is("SD_SAMPLER_TRAJ", "0"), !is("SD_SAMPLER_GEMM", "f32"), !is("SD_SAMPLER_TRAJG", "0"), mr ? atoi(mr) : 64,
                               !is("SD_TRAJ_ROLLOUT", "steps")};
    }();
    return sw;
}

// What a sampler call asks for besides its shape (a set of bits): the plan's rollout form depends on it, the route does not.
enum SamplerCall {
    CALL_ROLLOUT = 0,   // sd_ddim_sample*: the whole rollout, only its end is returned
    CALL_TRACE = 1,     // ... with the sample or the noise prediction of every step (trace / eps_trace)
    CALL_PIN = 2,       // ... with pinned leading rows (sd_ddim_sample_pin)
    CALL_LOOP = 4,      // the loop form: one denoiser evaluation per call (sd_sampler_eps)
};

struct SamplerPlan {
    int route;       // SD_ROUTE_*
    bool rollout_fused;   // TRAJ_TUNED / TRAJ_TUNED_2P: all DDIM steps of a trajectory in one launch (traj_step_rollout_kernel); false: one launch per step
    int key_tiles;   // tuned trajectory family: tiles of 16 memory slots in the folded blocks (1; 2 .. 4: the wide instantiation)
    bool precise;    // tuned trajectory family: three fp16 products at the Q | K | V site too (false: mode 4, which reports through the status word)
    bool kv_fp32;    // row panels: the memory's K / V projections stay on the fp32 MFMA (caps 0 and 1: the rerun path after SD_STATUS_NONFINITE)
    bool fused, fold, f16, chain16;   // row panels: fused layer kernel; folded cross-attention; decoder_layer_f16_kernel; chain_f16_kernel
    bool traj() const { return route >= SD_ROUTE_TRAJ_TUNED; }
    // the number sd_sampler_mode reports (4 is opt-in: never reported)
    int mode() const { return traj() ? 3 : route == SD_ROUTE_FUSED_FOLD_F16 ? 2 : route == SD_ROUTE_FUSED_FOLD ? 1 : 0; }
};

// The row-panel part of a plan: Mk memory rows per trajectory (the sampler's Mc + 1), cap 0 .. 2.
// fused and chain16 are not complements: a shape whose memory passes fused_layer_ok is never given the fp16 row chains, also where the
// size limit (the fused kernels index B * Mk * 2 d floats of K / V with 32 bits) then refuses the fused kernel - it runs the fp32 chains.
inline SamplerPlan panel_plan(int d, int heads, int T, int Mk, int J, int B, int cap) {
    const SamplerSwitches &sw = sampler_switches();
    const bool layer_ok = fused_layer_ok(d, heads, T, Mk);
    SamplerPlan p{};
    p.kv_fp32 = cap < 2;
    p.fused = layer_ok && (long)B * Mk * 2 * d < (1L << 30);
    // folded cross-attention: <= 16 key slots per head, <= 2 trajectories per panel
    p.fold = cap >= 1 && p.fused && heads == 4 && d >= 128 && Mk <= 16 && T >= 64;
    // the fp16x3 layer kernel is instantiated for hidden_dim 256, the fp16x3 row chains for 128 / 256 / 512
    p.f16 = cap >= 2 && p.fold && sw.f16 && d == 256 && J % 4 == 0;
    p.chain16 = cap >= 2 && !p.fold && !layer_ok && sw.f16 && (d == 128 || d == 256 || d == 512) && J % 4 == 0;
    p.route = p.f16 ? SD_ROUTE_FUSED_FOLD_F16 : p.fold ? SD_ROUTE_FUSED_FOLD : p.fused ? SD_ROUTE_FUSED : p.chain16 ? SD_ROUTE_CHAINS_F16 : SD_ROUTE_CHAINS_F32;
    return p;
}

// One sampler call: Mc context rows (+ the step row), L layers, B trajectories, max_mode already resolved to 0 .. 4.
// call: SamplerCall bits.  draws: trajectories per context (sd_ddim_sample_draws; B is a multiple of it) - the tuned kernels' folded blocks
// exist once per CONTEXT, so their size limit counts B / draws; everything else is a function of the same integers.
inline SamplerPlan sampler_plan(int d, int heads, int T, int Mc, int J, int L, int B, int max_mode, int call, int draws = 1) {
    const SamplerSwitches &sw = sampler_switches();
    const int Mk = Mc + 1;
    if (max_mode >= 3 && sw.traj && sw.f16) {
        // the tuned kernels take any horizon <= 100: they need the folded blocks, not the row-panel kernels' T >= 64
        if ((long)(B / (draws > 0 ? draws : 1)) * Mk * 2 * d < (1L << 30) && Mk <= sw.max_rows && traj_ok(d, heads, T, Mk, J, L)) {
            SamplerPlan p{};
            p.key_tiles = (Mk + 15) / 16;
            // more than 16 memory rows: the wide instantiation (three products everywhere, whatever the mode asked for)
            p.precise = max_mode == 3 || p.key_tiles > 1;
            p.route = p.key_tiles > 1 ? SD_ROUTE_TRAJ_TUNED_WIDE : p.precise ? SD_ROUTE_TRAJ_TUNED : SD_ROUTE_TRAJ_TUNED_2P;
            // the rollout kernel exists for the one-key-tile instantiations; it returns nothing per step and has no pinned twin
            p.rollout_fused = sw.rollout && p.key_tiles == 1 && call == CALL_ROLLOUT;
            return p;
        }
        if (sw.trajg && trajg_ok(d, heads, T, Mk, J, L)) {
            SamplerPlan p{};
            p.route = SD_ROUTE_TRAJ_GENERIC;
            return p;
        }
    }
    return panel_plan(d, heads, T, Mk, J, B, max_mode < 2 ? max_mode : 2);
}
#endif
