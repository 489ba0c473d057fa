// Run-time configuration: every knob of the library, its default, and the environment variable that overrides it -- each written ONCE.
//
// Precedence: config_defaults() < ripp_configure() < RIPP_* environment (a debug / A-B override).  config_resolve() applies the three in that
// order; the engine calls it once per C-ABI call (Engine::refresh_switches), never inside a proof, so a test or an A/B run flips a knob on a
// live engine.  A new knob takes a default in config_defaults(), a row in CONFIG_ENV, its use, and a row in DESIGN.md section 7b (a public one
// also a member of ripp_config in the header, Python and Rust).
// Two variables are deliberately NOT here because they are not per-call configuration: RIPP_HOST_WORKERS sizes the static host pool once, when
// it is created (engine.hip host_pool), and RIPP_TRACE is a process-wide diagnostic read once (engine.hip trace_on).
// Host only and free of the device runtime: besides the standard library this header needs include/ripp_hip.h alone, so a plain host compiler
// builds it (tests/host/config.cpp resolves configurations from stdin; tests/test_config_cpu.py checks every row of the table).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include "../../include/ripp_hip.h"

namespace ripp {

// What one call runs with.  `pub` is what ripp_config_get reports; the members behind it are deliberately not ABI.
struct Config {
    ripp_config pub;
    double ranks_per_device;          // the planner's value: RIPP_RANKS_PER_DEVICE=2.5 stays 2.5 here, pub.ranks_per_device reports 2
    uint32_t no_msm_batch;            // batched shared-base MSMs as a loop of single MSMs over the rows (A/B; the form the legacy MSM switches select too)
    uint32_t virtual_devices;         // RIPP_VIRTUAL_DEVICES=G (one-GPU test rig): pub.n_devices = G slots, all on the bound device
    // First-tier rounds of the transparent polynomial commitment (tpc_api.inc): key vectors of at least this length commit with the crossed two-row
    // batch pass, shorter ones with two single MSMs on two streams.  tools/tpc_first_tier_ab.py tabulates both forms per round length in
    // profiles/tpc_first_tier_ab.txt (crossed ahead at key length 4096, behind at 2048, level below); the bound has not been moved on that one table yet, so no
    // round takes the crossed form by default.  RIPP_TPC_CROSS_MIN overrides the bound per call (2: every round crossed).
    uint64_t tpc_cross_min;
    // Rounds of the TIPA prover for scalar products (tipa_scalar_api.inc): key vectors of at least this length commit with ONE crossed two-row pass of the batched
    // pipeline in G2 (tipa_scalar.hpp) followed by one in G1, shorter ones (and every round under the legacy MSM switches) with two single MSMs per group on two
    // side streams.  tools/tipa_scalar_ab.py tabulates both forms in profiles/tipa_scalar_ab.txt (whole proofs, n = 2^4 .. 2^16): the crossed form is within a few
    // per cent of the two-MSM form either way and NOT ahead at the longest measured size, so by the rule in that file's header no round takes it by default.
    // RIPP_TIPA_SCALAR_CROSS_MIN overrides the bound per call (2: every round crossed).
    uint64_t tipa_scalar_cross_min;
    // Rounds of the GIPA prover with a committed scalar vector (gipa_mexp_api.inc): vectors of at least this length run the round's four G1 MSMs as ONE
    // four-row pass of the batched pipeline (gipa_mexp.hpp), shorter ones as four single MSMs on two side streams.  profiles/gipa_mexp_ab.txt
    // (tools/gipa_mexp_ab.py): with every round in one pass the whole proof's median is below the four-MSM form's minimum at every measured n = 2^4 .. 2^16
    // (0.85 - 0.93 of it); 16 is the shortest measured length.  RIPP_GIPA_MEXP_BATCH_MIN overrides the bound per call (2: every round in one pass).
    uint64_t gipa_mexp_batch_min;
};

// The ONLY place a default value is written.  Members not named here default to 0: every selector, the MSM tuning triple (the plan's own
// choice), mem_cap_bytes, hot_workers, comm_timeout_ms, plan_derate_pct and n_devices (automatic: see ripp_hip.h).
inline Config config_defaults() {
    Config c{};
    ripp_config& p = c.pub;
    p.struct_size = (uint32_t)sizeof(ripp_config);
    p.look_eighths = -1;                             // the look-ahead plan chooses (cost model / adaptive)
    p.ranks_per_device = 1; c.ranks_per_device = 1.0;
    p.vm_lines_max = (uint64_t)1 << 15;              // launches with <= this many pairs use the 16-lanes-per-pair VM line kernel (measured crossover)
    p.vm_fold_max = (uint64_t)1 << 11;               // folds with <= this many outputs use the VM scalar multiplications
    p.vm_joint_max = (uint64_t)1 << 13;              // folds with <= this many outputs (and more than vm_fold_max) use the joint one-group-per-element VM forms
    p.vm_scale_max = (uint64_t)1 << 14;              // per-element G1 scalings of <= this many elements run on the VM (measured: direct product 6.1 -> 3.8 ms at 2^13, 7.1 -> 6.2 ms at 2^14, level at 2^15)
    p.vm_tree_max = (uint64_t)1 << 16;               // tree levels with <= this many products use the VM Fp12 multiplier
    p.gls_split_max = (uint64_t)1 << 14;             // rounds with <= this many outputs use the 4-lane GLS fold
    p.msm_vm_merge_max = 16384;                      // buckets (all windows) up to which the bucket merge runs on the field VM
    p.fold_tab_min = 32768;                          // G2 folds of at least this many elements build in-round odd-multiple tables
    p.fq_min = (uint64_t)1 << 15;                    // the carry-free fold kernels (fq_curve.hpp, fq_curve2.hpp): from 2^15 outputs (round 4 of an n = 2^20 proof: 5.4 -> 3.9 ms; below that the 12 x 32-bit forms have the shorter chains)
    p.lp_fq_min = 0;                                 // pairs per launch from which k_line_products_q replaces k_line_products: always (11 % faster per launch: 5.8 vs 6.5 ms at the proof's launch
                                                     // mix; it keeps ~47 dwords per lane in scratch, which costs HBM traffic, not time -- the kernel is issue-bound).  RIPP_LP_FQ_MIN=4294967295 / RIPP_NO_FQ select k_line_products
    p.ml_fq_min = 0;                                 // pairs per launch from which k_miller_lines_q (fq_miller.hpp) replaces k_miller_lines: every throughput launch (the VM kernel covers the small ones)
    p.fq_min_g1 = (uint64_t)1 << 12;                 // ... the G1 NAF fold (one 128-step chain per lane either way): the carry-free kernel wherever the lane-per-element form runs at all
    p.tail_pipe_max = (uint64_t)1 << 11;             // SIPP rounds of at most this length run pipelined (job_tail_enqueue); 0 = off
    p.msm_lds_sort_min = 0;                          // MSMs of >= this many terms (after the GLV / GLS split) sort through LDS tiles (msm.hpp k_msm_hist_lds / k_msm_scatter_lds); the lane-per-term sort below it (A/B)
    p.msm_chunk_min = (uint64_t)1 << 20;             // host-slice MSMs of >= this many G1 bases (half as many G2 bases: the same bytes) run as two halves on two streams (msm_impl: the second half's upload beside the first half's additions)
    c.tpc_cross_min = c.tipa_scalar_cross_min = ~(uint64_t)0;
    c.gipa_mexp_batch_min = 16;
    return c;
}

// One row per environment variable: how its value is read and the member it writes.  Rows apply in table order (a later row wins).
enum class EnvKind { FLAG, U32, U64, I32, SPECIAL };      // FLAG: 1 when the variable is present, WHATEVER its value (RIPP_NO_VM=0 switches the VM off); U32 / U64 / I32: decimal
struct ConfigEnvRow { const char* name; EnvKind kind; size_t off; const char* member; void (*special)(Config&, const char*); };
#define RIPP_ROW(name, kind, member) {name, EnvKind::kind, offsetof(Config, member), #member, nullptr}
#define RIPP_ROW_SPECIAL(name, member, fn) {name, EnvKind::SPECIAL, offsetof(Config, member), #member, [](Config& c, const char* s) fn}
inline const ConfigEnvRow CONFIG_ENV[] = {
    RIPP_ROW("RIPP_NO_VM", FLAG, pub.no_vm),
    RIPP_ROW("RIPP_NO_PRECOMPUTE", FLAG, pub.no_precompute),
    RIPP_ROW("RIPP_NO_FOLD_TABLES", FLAG, pub.no_fold_tables),
    RIPP_ROW("RIPP_NO_MSM_GLV", FLAG, pub.no_msm_glv),
    RIPP_ROW("RIPP_LP_ONE_LANE", FLAG, pub.lp_one_lane),
    RIPP_ROW("RIPP_NO_ENDO", FLAG, pub.no_endo),
    RIPP_ROW("RIPP_NO_FQ", FLAG, pub.no_fq),
    RIPP_ROW("RIPP_NO_XSCALE", FLAG, pub.no_xscale),
    RIPP_ROW("RIPP_SCALE_NO_FQ", FLAG, pub.scale_no_fq),
    RIPP_ROW("RIPP_AGG_SEQUENTIAL", FLAG, pub.agg_sequential),
    RIPP_ROW("RIPP_LOOK_STATIC", FLAG, pub.look_static),
    RIPP_ROW("RIPP_QUIET_WAITS", FLAG, pub.quiet_waits),
    RIPP_ROW("RIPP_NO_SHARE", FLAG, pub.no_share),
    RIPP_ROW("RIPP_NO_FUSE", FLAG, pub.no_fuse),
    RIPP_ROW("RIPP_FUSE_TABLES", FLAG, pub.fuse_tables),
    RIPP_ROW("RIPP_NO_PREBUILD", FLAG, pub.no_prebuild),
    RIPP_ROW("RIPP_NO_JOB_CACHE", FLAG, pub.no_job_cache),
    RIPP_ROW("RIPP_NO_LP_KARA", FLAG, pub.no_lp_karatsuba),
    RIPP_ROW("RIPP_NO_MSM_BATCH", FLAG, no_msm_batch),
    RIPP_ROW_SPECIAL("RIPP_LOOK_ITEMS", pub.look_eighths, { c.pub.look_eighths = 8 * std::max(0, std::atoi(s)); }),      // whole (round, side) items
    RIPP_ROW_SPECIAL("RIPP_LOOK_EIGHTHS", pub.look_eighths, { c.pub.look_eighths = std::max(0, std::atoi(s)); }),       // 8 k + f: k items and f/8 of the next
    RIPP_ROW_SPECIAL("RIPP_RANKS_PER_DEVICE", ranks_per_device, { c.ranks_per_device = std::max(1.0, std::atof(s)); }),
    RIPP_ROW("RIPP_MSM_C", I32, pub.msm_c),
    RIPP_ROW("RIPP_MSM_CH", U32, pub.msm_ch),
    RIPP_ROW("RIPP_MSM_GMIN", U32, pub.msm_gmin),
    RIPP_ROW("RIPP_VM_LINES_MAX", U64, pub.vm_lines_max),
    RIPP_ROW("RIPP_VM_FOLD_MAX", U64, pub.vm_fold_max),
    RIPP_ROW("RIPP_VM_TREE_MAX", U64, pub.vm_tree_max),
    RIPP_ROW("RIPP_GLS_SPLIT_MAX", U64, pub.gls_split_max),
    RIPP_ROW("RIPP_MSM_VM_MERGE_MAX", U64, pub.msm_vm_merge_max),
    RIPP_ROW("RIPP_FOLD_TAB_MIN", U64, pub.fold_tab_min),
    RIPP_ROW("RIPP_FQ_MIN", U64, pub.fq_min),
    RIPP_ROW("RIPP_LP_FQ_MIN", U64, pub.lp_fq_min),
    RIPP_ROW("RIPP_VM_JOINT_MAX", U64, pub.vm_joint_max),
    RIPP_ROW("RIPP_VM_SCALE_MAX", U64, pub.vm_scale_max),
    RIPP_ROW("RIPP_TAIL_PIPE_MAX", U64, pub.tail_pipe_max),
    RIPP_ROW("RIPP_ML_FQ_MIN", U64, pub.ml_fq_min),
    RIPP_ROW("RIPP_FQ_MIN_G1", U64, pub.fq_min_g1),
    RIPP_ROW("RIPP_MSM_LDS_SORT_MIN", U64, pub.msm_lds_sort_min),
    RIPP_ROW("RIPP_MSM_CHUNK_MIN", U64, pub.msm_chunk_min),
    RIPP_ROW("RIPP_MEM_CAP_BYTES", U64, pub.mem_cap_bytes),
    RIPP_ROW_SPECIAL("RIPP_HOT_WORKERS", pub.hot_workers, { c.pub.hot_workers = std::atoi(s) ? 1 : 2; }),               // non-zero: always, 0: never
    RIPP_ROW("RIPP_COMM_TIMEOUT_MS", U32, pub.comm_timeout_ms),
    RIPP_ROW("RIPP_PLAN_DERATE_PCT", U32, pub.plan_derate_pct),
    RIPP_ROW("RIPP_N_DEVICES", U32, pub.n_devices),
    RIPP_ROW_SPECIAL("RIPP_VIRTUAL_DEVICES", pub.n_devices, { c.pub.n_devices = (uint32_t)std::strtoul(s, nullptr, 10); c.virtual_devices = 1; }),
    RIPP_ROW("RIPP_TPC_CROSS_MIN", U64, tpc_cross_min),
    RIPP_ROW("RIPP_TIPA_SCALAR_CROSS_MIN", U64, tipa_scalar_cross_min),
    RIPP_ROW("RIPP_GIPA_MEXP_BATCH_MIN", U64, gipa_mexp_batch_min),
};
#undef RIPP_ROW
#undef RIPP_ROW_SPECIAL

// defaults, then `configured` (ripp_configure's struct, or null), then the environment as `env` (std::getenv, or a test's map) reports it
template <class GetEnv> inline Config config_resolve(const ripp_config* configured, GetEnv&& env) {
    Config c = config_defaults();
    if (configured) { c.pub = *configured; c.ranks_per_device = c.pub.ranks_per_device > 1 ? (double)c.pub.ranks_per_device : 1.0; }
    for (const ConfigEnvRow& r : CONFIG_ENV) {
        const char* s = env(r.name);
        char* m = reinterpret_cast<char*>(&c) + r.off;
        if (r.kind == EnvKind::FLAG) { uint32_t& v = *reinterpret_cast<uint32_t*>(m); v = s || v; }      // (a configured selector reads back as 0 / 1 too)
        else if (!s) continue;
        else if (r.kind == EnvKind::U32) *reinterpret_cast<uint32_t*>(m) = (uint32_t)std::strtoul(s, nullptr, 10);
        else if (r.kind == EnvKind::U64) *reinterpret_cast<uint64_t*>(m) = (uint64_t)std::strtoull(s, nullptr, 10);
        else if (r.kind == EnvKind::I32) *reinterpret_cast<int32_t*>(m) = (int32_t)std::atoi(s);
        else r.special(c, s);
    }
    c.pub.ranks_per_device = (int32_t)c.ranks_per_device;
#if !defined(RIPP_AB_KERNELS) || defined(RIPP_BLS12_377)
    c.pub.lp_one_lane = 0;                           // k_line_products1 is compiled into A/B builds of the BLS12-381 library only (-DRIPP_AB_KERNELS)
#endif
    return c;
}
// ... from the process environment: the library's only reader of RIPP_* configuration
inline Config config_resolve(const ripp_config* configured) { return config_resolve(configured, [](const char* k) { return std::getenv(k); }); }

}  // namespace ripp
