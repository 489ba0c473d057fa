"""CPU: the run-time configuration of ripp_amd/csrc/config.hpp -- one table, one resolver -- as pure host code.
tests/host/config.cpp is built stand-alone (plain, -DRIPP_BLS12_377, -DRIPP_AB_KERNELS, and the two together) and resolves the cases it reads on stdin
with a map in place of the process environment.  Checked, for every row of the table the program prints and for every build:
  defaults    with nothing set every member has the value written out in DEFAULTS below (what ripp_config_default returned before the table existed)
  rows        the variable alone, and the configured member alone, change exactly that row's member(s); the environment wins over ripp_configure;
              a case without a configured struct shows none of an earlier case's values
  specials    RIPP_LOOK_ITEMS / RIPP_LOOK_EIGHTHS / RIPP_HOT_WORKERS / RIPP_RANKS_PER_DEVICE / RIPP_VIRTUAL_DEVICES, flags that are set by their presence,
              lp_one_lane outside the A/B build of the BLS12-381 library
  complete    the "RIPP_..." literals of config.hpp are the table; every row is documented in DESIGN.md section 7b; nothing else in csrc reads the environment
and the whole input once more through an AddressSanitizer + UBSan build of the same stand-alone program."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ripp_amd", "csrc")
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
BUILDS = {"plain": [], "377": ["-DRIPP_BLS12_377"], "ab": ["-DRIPP_AB_KERNELS"], "ab377": ["-DRIPP_AB_KERNELS", "-DRIPP_BLS12_377"]}
ONE_LANE_BUILDS = ("ab",)                   # k_line_products1 exists in A/B builds of the BLS12-381 library only

SELECTORS = ("no_vm", "no_precompute", "no_fold_tables", "no_msm_glv", "lp_one_lane", "no_endo", "no_fq", "no_xscale", "scale_no_fq", "agg_sequential", "look_static",
             "quiet_waits", "no_share", "no_fuse", "fuse_tables", "no_prebuild", "no_job_cache", "no_lp_karatsuba")
DEFAULTS = {"pub.struct_size": 240,      # tests/test_abi_cpu.py pins sizeof(ripp_config)
            "pub.vm_lines_max": 1 << 15, "pub.vm_fold_max": 1 << 11, "pub.vm_tree_max": 1 << 16, "pub.gls_split_max": 1 << 14, "pub.msm_vm_merge_max": 16384,
            "pub.fold_tab_min": 32768, "pub.fq_min": 1 << 15, "pub.lp_fq_min": 0, "pub.vm_joint_max": 1 << 13, "pub.vm_scale_max": 1 << 14, "pub.tail_pipe_max": 1 << 11,
            "pub.ml_fq_min": 0, "pub.fq_min_g1": 1 << 12, "pub.msm_lds_sort_min": 0, "pub.msm_chunk_min": 1 << 20, "pub.look_eighths": -1, "pub.ranks_per_device": 1,
            "ranks_per_device": 1.0, "pub.msm_c": 0, "pub.msm_ch": 0, "pub.msm_gmin": 0, "pub.mem_cap_bytes": 0, "pub.hot_workers": 0, "pub.comm_timeout_ms": 0,
            "pub.plan_derate_pct": 0, "pub.n_devices": 0, "no_msm_batch": 0, "virtual_devices": 0, "tpc_cross_min": 2**64 - 1, "tipa_scalar_cross_min": 2**64 - 1,
            "gipa_mexp_batch_min": 16, **{"pub." + s: 0 for s in SELECTORS}}

# SPECIAL rows: (value in the environment, what it gives), (configured value of the row's member, what it gives)
SPECIAL = {
    "RIPP_LOOK_ITEMS": (("3", {"pub.look_eighths": 24}), (9, {"pub.look_eighths": 9})),
    "RIPP_LOOK_EIGHTHS": (("5", {"pub.look_eighths": 5}), (9, {"pub.look_eighths": 9})),
    "RIPP_RANKS_PER_DEVICE": (("3", {"ranks_per_device": 3.0, "pub.ranks_per_device": 3}), (4, {"ranks_per_device": 4.0, "pub.ranks_per_device": 4})),
    "RIPP_HOT_WORKERS": (("7", {"pub.hot_workers": 1}), (2, {"pub.hot_workers": 2})),
    "RIPP_VIRTUAL_DEVICES": (("4", {"pub.n_devices": 4, "virtual_devices": 1}), (3, {"pub.n_devices": 3})),
}


def _compile(tmp, name, flags):
    exe = os.path.join(tmp, "config_" + name)
    subprocess.check_call([CLANG, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror"] + flags + ["-I" + CSRC, os.path.join(ROOT, "tests", "host", "config.cpp"), "-o", exe])
    return exe


def _resolve(exe, cases):
    """cases: (environment dict, configured dict or None) -> the table's rows and one {member: value} per case"""
    text = ""
    for env, cfg in cases:
        text += "".join("%s=%s\n" % kv for kv in env.items())
        if cfg is not None:
            text += "cfg\n" + "".join("cfg.%s=%d\n" % (k[4:] if k.startswith("pub.") else k, v) for k, v in cfg.items())
        text += "--\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[0].split()[0] == "TABLE"
    table = [tuple(w.split(":")) for w in out[0].split()[1:]]
    results, cur = [], {}
    for ln in out[1:]:
        if ln == "--":
            results.append(cur); cur = {}
            continue
        k, v = ln.split("=")
        assert k not in cur, "printed twice: " + k
        cur[k] = float(v) if k == "ranks_per_device" else int(v)
    assert len(results) == len(cases) and not cur
    return table, results


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("config"))
    return {name: _compile(tmp, name, flags) for name, flags in BUILDS.items()}


def _expect(build, changes):
    e = dict(DEFAULTS); e.update(changes)
    if build not in ONE_LANE_BUILDS: e["pub.lp_one_lane"] = 0
    return e


def _row_cases(table, build):
    """(label, environment, configured, expected members) for every row: the variable alone, the member alone, both (different values), then neither"""
    cases = [("nothing set", {}, None, _expect(build, {})), ("the defaults configured", {}, {}, _expect(build, {}))]
    for name, kind, member in table:
        if kind == "SPECIAL": (env_v, env_x), (cfg_v, cfg_x) = SPECIAL[name]
        elif kind == "FLAG": (env_v, env_x), (cfg_v, cfg_x) = ("1", {member: 1}), (1, {member: 1})
        else: (env_v, env_x), (cfg_v, cfg_x) = ("12345", {member: 12345}), (777, {member: 777})
        cfg_member = "pub.ranks_per_device" if name == "RIPP_RANKS_PER_DEVICE" else member
        cases.append((name + " alone", {name: env_v}, None, _expect(build, env_x)))
        if cfg_member.startswith("pub."):                        # rows with an ABI member
            cases.append((cfg_member + " configured", {}, {cfg_member: cfg_v}, _expect(build, cfg_x)))
            other = 0 if kind == "FLAG" else cfg_v             # a flag that is configured OFF is still switched on by its variable
            cases.append((name + " over " + cfg_member, {name: env_v}, {cfg_member: other}, _expect(build, env_x)))
            cases.append(("nothing after " + cfg_member, {}, None, _expect(build, {})))
    return cases


SPECIAL_CASES = [      # (environment, configured, members that differ from the defaults) -- on a build with lp_one_lane these are build-independent
    ({"RIPP_LOOK_ITEMS": "3"}, None, {"pub.look_eighths": 24}),
    ({"RIPP_LOOK_ITEMS": "-2"}, None, {"pub.look_eighths": 0}),
    ({"RIPP_LOOK_EIGHTHS": "-5"}, None, {"pub.look_eighths": 0}),
    ({"RIPP_LOOK_ITEMS": "3", "RIPP_LOOK_EIGHTHS": "5"}, None, {"pub.look_eighths": 5}),
    ({"RIPP_LOOK_EIGHTHS": "5", "RIPP_LOOK_ITEMS": "3"}, None, {"pub.look_eighths": 5}),
    ({"RIPP_HOT_WORKERS": "0"}, None, {"pub.hot_workers": 2}),
    ({"RIPP_HOT_WORKERS": "7"}, None, {"pub.hot_workers": 1}),
    ({"RIPP_HOT_WORKERS": "0"}, {"pub.hot_workers": 1}, {"pub.hot_workers": 2}),
    ({"RIPP_RANKS_PER_DEVICE": "0.5"}, None, {}),
    ({"RIPP_RANKS_PER_DEVICE": "2.5"}, None, {"ranks_per_device": 2.5, "pub.ranks_per_device": 2}),
    ({"RIPP_RANKS_PER_DEVICE": "2.5"}, {"pub.ranks_per_device": 8}, {"ranks_per_device": 2.5, "pub.ranks_per_device": 2}),
    ({}, {"pub.ranks_per_device": 0}, {}),
    ({}, {"pub.ranks_per_device": -3}, {}),
    ({"RIPP_N_DEVICES": "2", "RIPP_VIRTUAL_DEVICES": "4"}, None, {"pub.n_devices": 4, "virtual_devices": 1}),
    ({"RIPP_VIRTUAL_DEVICES": "4", "RIPP_N_DEVICES": "2"}, {"pub.n_devices": 8}, {"pub.n_devices": 4, "virtual_devices": 1}),
    ({"RIPP_N_DEVICES": "2"}, {"pub.n_devices": 8}, {"pub.n_devices": 2}),
    ({"RIPP_NO_VM": "0"}, None, {"pub.no_vm": 1}),
    ({"RIPP_NO_MSM_BATCH": ""}, None, {"no_msm_batch": 1}),
    ({}, {"pub.no_fq": 7}, {"pub.no_fq": 1}),                    # a selector reads back as 0 / 1
    ({"RIPP_MSM_C": "-3"}, None, {"pub.msm_c": -3}),
    ({"RIPP_MEM_CAP_BYTES": str(40 << 30)}, None, {"pub.mem_cap_bytes": 40 << 30}),      # above 2^32
    ({"RIPP_LP_FQ_MIN": "4294967295", "RIPP_TAIL_PIPE_MAX": "0"}, {"pub.tail_pipe_max": 64, "pub.look_eighths": 24}, {"pub.lp_fq_min": 4294967295, "pub.tail_pipe_max": 0, "pub.look_eighths": 24}),
]


def _check(exe, cases):
    table, results = _resolve(exe, [(env, cfg) for _, env, cfg, _ in cases])
    for (label, _, _, want), got in zip(cases, results):
        assert got == want, (label, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)})
    return table


@pytest.mark.parametrize("build", list(BUILDS))
def test_defaults_and_every_row_of_the_table(exes, build):
    table, _ = _resolve(exes[build], [])
    assert len({n for n, _, _ in table}) == len(table)
    assert {k for _, k, _ in table} == {"FLAG", "U32", "U64", "I32", "SPECIAL"} and {n for n, k, _ in table if k == "SPECIAL"} == set(SPECIAL)
    members = {m for _, _, m in table}
    assert members | {"pub.struct_size", "pub.ranks_per_device", "virtual_devices"} == set(DEFAULTS), "a member without a row, or a row without a default in this test"
    _check(exes[build], _row_cases(table, build))


@pytest.mark.parametrize("build", list(BUILDS))
def test_special_rows_and_the_order_they_apply_in(exes, build):
    _check(exes[build], [(repr((env, cfg)), env, cfg, _expect(build, x)) for env, cfg, x in SPECIAL_CASES])


def test_lp_one_lane_survives_only_in_the_ab_build_of_bls12_381(exes):
    for build in BUILDS:
        _, (by_env, by_cfg) = _resolve(exes[build], [({"RIPP_LP_ONE_LANE": "1"}, None), ({}, {"pub.lp_one_lane": 1})])
        want = 1 if build == "ab" else 0
        assert (by_env["pub.lp_one_lane"], by_cfg["pub.lp_one_lane"]) == (want, want), build


def _csrc_files():
    for d, _, fs in os.walk(CSRC):
        for f in fs:
            yield os.path.join(d, f)


def test_the_table_is_complete(exes):
    table, _ = _resolve(exes["plain"], [])
    names = [n for n, _, _ in table]
    literals = re.findall(r'"(RIPP_[A-Z0-9_]+)"', open(os.path.join(CSRC, "config.hpp")).read())
    assert sorted(literals) == sorted(names), "a RIPP_ literal of config.hpp that is no row of CONFIG_ENV (or a row written twice)"
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = design[design.index("### 7b."):]
    sec = sec[:sec.index("\n## ")]
    rows = [ln for ln in sec.splitlines() if ln.startswith("|")]
    documented = set(re.findall(r"`(RIPP_[A-Z0-9_]+)", "\n".join(ln.split("|")[1] for ln in rows)))
    assert set(names) <= documented, sorted(set(names) - documented)
    assert "\n\n|" not in sec[sec.index("\n|"):], "DESIGN.md section 7b has a second table"
    # the environment is read in config.hpp and, outside the table on purpose, for RIPP_HOST_WORKERS and RIPP_TRACE (both read once per process)
    sites = [(os.path.relpath(p, CSRC), ln.strip()) for p in _csrc_files() for ln in open(p, errors="replace") if "getenv" in ln and os.path.basename(p) != "config.hpp"]
    assert len(sites) == 2 and all(f == "engine.hip" for f, _ in sites), sites
    assert sorted(re.findall(r'getenv\("(\w+)"\)', " ".join(ln for _, ln in sites))) == ["RIPP_HOST_WORKERS", "RIPP_TRACE"]
    gone = [p for p in _csrc_files() if re.search(r"Sizes\{|struct Switches|config_from_engine", open(p, errors="replace").read())]
    assert not gone, gone


def test_the_whole_input_under_address_and_undefined_behaviour_sanitizers(exes, tmp_path):
    """the stand-alone program itself is the sanitized binary (no preload, nothing loaded into python, no device)"""
    exe = _compile(str(tmp_path), "san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DRIPP_AB_KERNELS"])
    table, _ = _resolve(exes["ab"], [])
    _check(exe, _row_cases(table, "ab") + [(repr((env, cfg)), env, cfg, _expect("ab", x)) for env, cfg, x in SPECIAL_CASES])
