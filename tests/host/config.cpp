// Stand-alone driver of ripp_amd/csrc/config.hpp (tests/test_config_cpu.py): resolves configurations described on stdin and prints every member.
//
// Input: cases separated by a line "--".  In a case, "NAME=VALUE" sets an environment variable (of this case only: the "environment" is a map
// handed to config_resolve, never the process's), "cfg.member=value" sets a member of the struct passed as `configured` (which starts from
// config_defaults().pub; a bare "cfg" line passes the defaults themselves), and without any cfg line `configured` is null.
// Output: one line "TABLE" with name:KIND:member of every row of CONFIG_ENV, then per case one "member=value" line per member and a line "--".
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <map>
#include <string>
#include "config.hpp"

using namespace ripp;

// every member of ripp_config (the static_assert below notices a missing one: the struct has no padding) and of the non-ABI tail of Config
#define PUB_MEMBERS(X) X(struct_size) X(no_vm) X(no_precompute) X(no_fold_tables) X(no_msm_glv) X(lp_one_lane) X(no_endo) X(no_fq) X(no_xscale) X(scale_no_fq) X(agg_sequential) \
    X(look_static) X(quiet_waits) X(no_share) X(no_fuse) X(fuse_tables) X(look_eighths) X(ranks_per_device) X(msm_c) X(msm_ch) X(msm_gmin) X(no_prebuild) \
    X(vm_lines_max) X(vm_fold_max) X(vm_tree_max) X(gls_split_max) X(msm_vm_merge_max) X(fold_tab_min) X(fq_min) X(lp_fq_min) X(vm_joint_max) X(vm_scale_max) X(tail_pipe_max) \
    X(ml_fq_min) X(fq_min_g1) X(msm_lds_sort_min) X(msm_chunk_min) X(mem_cap_bytes) X(hot_workers) X(no_job_cache) X(no_lp_karatsuba) X(comm_timeout_ms) X(plan_derate_pct) X(n_devices)
#define TAIL_MEMBERS(X) X(no_msm_batch) X(virtual_devices) X(tpc_cross_min) X(tipa_scalar_cross_min) X(gipa_mexp_batch_min)
#define SIZE_OF(m) + sizeof(ripp_config::m)
static_assert(0 PUB_MEMBERS(SIZE_OF) == sizeof(ripp_config), "PUB_MEMBERS does not list every member of ripp_config");

static void print(const char* name, uint32_t v) { std::printf("%s=%" PRIu32 "\n", name, v); }
static void print(const char* name, int32_t v) { std::printf("%s=%" PRId32 "\n", name, v); }
static void print(const char* name, uint64_t v) { std::printf("%s=%" PRIu64 "\n", name, v); }
static void assign(uint32_t& m, const std::string& v) { m = (uint32_t)std::stoull(v); }
static void assign(int32_t& m, const std::string& v) { m = (int32_t)std::stoll(v); }
static void assign(uint64_t& m, const std::string& v) { m = (uint64_t)std::stoull(v); }

static bool set_member(ripp_config& c, const std::string& name, const std::string& value) {
#define SET(m) if (name == #m) { assign(c.m, value); return true; }
    PUB_MEMBERS(SET)
#undef SET
    return false;
}

static void run_case(const std::map<std::string, std::string>& env, const ripp_config* configured) {
    const Config c = config_resolve(configured, [&env](const char* k) -> const char* { auto it = env.find(k); return it == env.end() ? nullptr : it->second.c_str(); });
#define PRINT_PUB(m) print("pub." #m, c.pub.m);
#define PRINT_TAIL(m) print(#m, c.m);
    PUB_MEMBERS(PRINT_PUB)
    std::printf("ranks_per_device=%.17g\n", c.ranks_per_device);
    TAIL_MEMBERS(PRINT_TAIL)
    std::printf("--\n");
}

int main() {
    static const char* const KIND[] = {"FLAG", "U32", "U64", "I32", "SPECIAL"};
    std::printf("TABLE");
    for (const ConfigEnvRow& r : CONFIG_ENV) std::printf(" %s:%s:%s", r.name, KIND[(int)r.kind], r.member);
    std::printf("\n");
    std::map<std::string, std::string> env; ripp_config configured = config_defaults().pub; bool have_cfg = false, open = false;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line == "--") { run_case(env, have_cfg ? &configured : nullptr); env.clear(); configured = config_defaults().pub; have_cfg = open = false; continue; }
        if (line.empty()) continue;
        open = true;
        const size_t eq = line.find('=');
        if (line == "cfg") have_cfg = true;
        else if (eq == std::string::npos) { std::fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
        else if (line.compare(0, 4, "cfg.") == 0) {
            have_cfg = true;
            if (!set_member(configured, line.substr(4, eq - 4), line.substr(eq + 1))) { std::fprintf(stderr, "no such member: %s\n", line.c_str()); return 2; }
        } else env[line.substr(0, eq)] = line.substr(eq + 1);
    }
    if (open) run_case(env, have_cfg ? &configured : nullptr);
    return 0;
}
