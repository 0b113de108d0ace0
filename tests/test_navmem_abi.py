"""Who exports the live layer with memory (include/ssf_navmem.h), without a GPU: libssf_hip_mem.so holds libssf_hip_dyn.so's symbols and
exactly the two new entry points and the k_navmem_* kernels; the ten other libraries and the oracle hold no name of it; the product's
table is the golden one; the header stands on its own and the binding's structures have its layout."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import navmem_ref as mr
from conftest import ROOT
from supersurfel_fusion_amd import binding

INCLUDE = os.path.join(ROOT, "include")
OLDER = ("NAVCARVE_LIB", "NAV_LIB", "EXPLORE_LIB", "DRIVE_LIB", "LIVE_LIB", "STEER_LIB", "FOOT_LIB", "POSE_LIB", "DYN_LIB")


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


@pytest.fixture(scope="module")
def mem_lib(product_lib):
    return binding.load_mem()


def test_the_mem_library_exports_its_own_symbols_and_all_of_the_dyn_library(mem_lib, product_lib, oracle_lib):
    have, dyn = exported(mem_lib.path), exported(binding.DYN_LIB)
    hip_ids = lambda names: {nm for nm in names if nm.startswith("__hip_cuid_")}         # one per translation unit, named by content
    for names in (binding.NAVMEM_SYMBOLS, binding.NAVDYN_SYMBOLS, binding.NAVPOSE_SYMBOLS, binding.NAVFOOT_SYMBOLS, binding.NAVSTEER_SYMBOLS,
                  binding.NAVLIVE_SYMBOLS, binding.NAVPATH_SYMBOLS, binding.NAVFRONTIER_SYMBOLS, binding.NAVPLAN_SYMBOLS, binding.NAVCARVE_SYMBOLS,
                  binding.ABI_SYMBOLS):
        assert set(names) <= have
    assert mem_lib.has_navmem and mem_lib.has_navdyn and mem_lib.has_navlive and mem_lib.backend == "hip-gfx950"
    assert dyn - hip_ids(dyn) <= have
    extra = have - dyn - hip_ids(have)
    assert binding.NAVMEM_SYMBOLS == ["ssf_navmem_default_params", "ssf_navmem_update"] and set(binding.NAVMEM_SYMBOLS) <= extra
    kernels = extra - set(binding.NAVMEM_SYMBOLS)
    assert kernels == {nm for nm in extra if "k_navmem_" in nm}, sorted(extra)
    for k in ("k_navmem_stamp", "k_navmem_march", "k_navmem_cells"):
        assert any(k in nm for nm in kernels), k


def test_no_other_library_holds_a_name_of_it(product_lib, oracle_lib):
    for other in [exported(product_lib.path), exported(oracle_lib.path)] + [exported(getattr(binding, nm)) for nm in OLDER]:
        assert not [nm for nm in other if "navmem" in nm]
    for load in ("load_navcarve", "load_nav", "load_explore", "load_drive", "load_live", "load_steer", "load_foot", "load_pose", "load_dyn"):
        assert not getattr(binding, load)().has_navmem
    assert not product_lib.has_navmem and not oracle_lib.has_navmem


def test_the_products_table_is_the_golden_one(product_lib):
    want = open(os.path.join(ROOT, "tests", "golden", "libssf_hip_dynsyms.txt")).read().split()
    have = sorted(exported(product_lib.path))
    assert have == sorted(want), sorted(set(have) ^ set(want))


def test_an_older_library_names_the_missing_symbol(product_lib):
    lib = binding.load_dyn()
    assert not lib.has_navmem
    f = binding.Fusion.__new__(binding.Fusion)                            # (no handle: the check comes before any call)
    f.L = lib
    state, depth = np.zeros((3, 3), np.int8), np.ones((48, 64), np.float32)
    with pytest.raises(binding.SsfError, match="ssf_navmem_update.*binding.load_mem"):
        f.nav_memory(depth, state)
    with pytest.raises(binding.SsfError, match="ssf_navmem_update.*binding.load_mem"):
        f.nav_memory_device(0, 0, 3, 3)
    with pytest.raises(binding.SsfError, match="ssf_navmem_default_params.*binding.load_mem"):
        f.nav_memory_default_params()
    with pytest.raises(binding.SsfError, match="ssf_navmem_update.*binding.load_mem"):
        f.nav_memory_plan(depth, state, None, [(1, 1)], [(1, 1)])
    with pytest.raises(binding.SsfError, match="ssf_navmem_update.*binding.load_mem"):
        f.nav_memory_dyn_steer(depth, state, None, [(1, 1)], np.zeros((1, 3), np.int32), binding.MoverTracker())


def test_the_symbols_stay_out_of_the_other_headers():
    for nm in binding.NAVMEM_SYMBOLS:
        assert nm not in binding.ABI_SYMBOLS
        for hdr in sorted(os.listdir(INCLUDE)):
            if hdr.endswith(".h") and hdr != "ssf_navmem.h":
                assert nm not in open(os.path.join(INCLUDE, hdr)).read(), (nm, hdr)
        assert nm + "(" in open(os.path.join(INCLUDE, "ssf_navmem.h")).read()
    assert "#define SSF_ABI_VERSION 3" in open(os.path.join(INCLUDE, "ssf.h")).read()


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_the_header_compiles_on_its_own_and_the_binding_has_its_layout(lang, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    fields = lambda st: ", ".join("(int)offsetof(%s, %s)" % (st[0], nm) for nm, _ in st[1]._fields_)
    structs = (("ssf_navmem_params", binding.SsfNavMemParams), ("ssf_navmem_layer", binding.SsfNavMemLayer), ("ssf_navmem_out", binding.SsfNavMemOut),
               ("ssf_navmem_stats", binding.SsfNavMemStats))
    body = "".join('    printf("%s %%d", (int)sizeof(%s));\n    { int o[] = {%s}; for (unsigned i = 0; i < sizeof(o) / sizeof(o[0]); i++) printf(" %%d", o[i]); }\n'
                   '    printf("\\n");\n' % (st[0], st[0], fields(st)) for st in structs)
    src.write_text('#include "ssf_navmem.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n' + body + "    return 0;\n}\n")
    exe = str(tmp_path / "t")
    r = subprocess.run(["gcc" if lang == "c" else "g++", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, str(src), "-o", exe], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    for (name, st), line in zip(structs, lines):
        got = [int(v) for v in line.split()[1:]]
        assert line.split()[0] == name and got == [C.sizeof(st)] + [getattr(st, nm).offset for nm, _ in st._fields_], (name, line)


def test_the_binding_names_what_the_restatement_names():
    assert binding.NAVMEM_OUTPUT_NAMES == mr.OUTPUTS and binding.NAVMEM_LAYER_NAMES == mr.LAYER
    assert tuple(nm for nm, _ in binding.SsfNavMemStats._fields_) == mr.STATS + ("atomics", "pose")
    hdr = open(os.path.join(INCLUDE, "ssf_navmem.h")).read()
    for nm, _ in binding.SsfNavMemParams._fields_:
        assert re.search(r"\b%s\b" % nm, hdr), nm
    assert "min_seen" not in dict(binding.SsfNavMemParams._fields_)


def test_live_memory_keeps_the_layer_and_the_tick():
    mem = binding.LiveMemory(5, 3)
    assert [a.shape for a in mem.arrays()] == [(3, 5)] * 3 and all(a.dtype == np.uint32 and not a.any() for a in mem.arrays()) and mem.tick == 0
    assert mem.next_tick() == 1 and mem.next_tick(9) == 9
    mem.tick = 0xFFFFFFFF
    assert mem.next_tick() == 1                                          # the tick skips 0 when it wraps
    mem.marks[1, 2] = 7
    keep = mem.marks
    mem.clear()
    assert mem.marks is keep and not mem.marks.any() and mem.tick == 0
    for bad in (0, -1, 1 << 32):
        with pytest.raises(binding.SsfError, match="tick"):
            mem.next_tick(bad)
    with pytest.raises(binding.SsfError, match="width and height"):
        binding.LiveMemory(0, 3)


def test_the_replay_options_parse():
    from supersurfel_fusion_amd import replay
    base = ["--npz", "frames.npz", "--nav-grid-dir", "grids"]
    a = replay.parse_args(base + ["--nav-live", "--nav-live-memory"])
    assert replay.nav_live_of(a) == dict(min_hits=4, stride=4, memory=dict(forget=0, slices=16)) and replay.library_of(a) == "load_mem"
    a = replay.parse_args(base + ["--nav-live", "--nav-live-memory", "--nav-live-forget", "30", "--nav-live-slices", "8", "--nav-live-stride", "8",
                                  "--nav-plan-goal", "1.0", "2.0", "--nav-steer", "--nav-steer-movers"])
    assert replay.nav_live_of(a) == dict(min_hits=4, stride=8, memory=dict(forget=30, slices=8)) and replay.library_of(a) == "load_mem"
    a = replay.parse_args(base + ["--nav-live"])                         # without it: as before
    assert replay.nav_live_of(a) == dict(min_hits=4, stride=4) and replay.library_of(a) == "load_live"
    for bad in (["--nav-live-memory"], ["--nav-live", "--nav-live-forget", "3"], ["--nav-live", "--nav-live-slices", "8"],
                ["--nav-live", "--nav-live-memory", "--nav-live-slices", "0"], ["--nav-live", "--nav-live-memory", "--nav-live-slices", "33"],
                ["--nav-live", "--nav-live-memory", "--nav-live-forget", "-1"]):
        with pytest.raises(SystemExit):
            replay.parse_args(base + bad)
