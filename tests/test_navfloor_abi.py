"""Who exports the fitted floor plane (include/ssf_navfloor.h), without a GPU: libssf_hip_floor.so holds libssf_hip_mem.so's symbols and
exactly the two new entry points and the k_navfloor_* kernels; the eleven other libraries and the oracle hold no name of it; the
product's table is the golden one; the header stands on its own and the binding's structures have its layout; the replay options parse."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import navfloor_ref as fr
from conftest import ROOT
from supersurfel_fusion_amd import binding

INCLUDE = os.path.join(ROOT, "include")
OLDER = ("NAVCARVE_LIB", "NAV_LIB", "EXPLORE_LIB", "DRIVE_LIB", "LIVE_LIB", "STEER_LIB", "FOOT_LIB", "POSE_LIB", "DYN_LIB", "MEM_LIB")


def exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    return {l.split()[-1] for l in out.splitlines() if l.strip()}


@pytest.fixture(scope="module")
def floor_lib(product_lib):
    return binding.load_floor()


def test_the_floor_library_exports_its_own_symbols_and_all_of_the_mem_library(floor_lib, product_lib, oracle_lib):
    have, mem = exported(floor_lib.path), exported(binding.MEM_LIB)
    hip_ids = lambda names: {nm for nm in names if nm.startswith("__hip_cuid_")}         # one per translation unit, named by content
    for names in (binding.NAVFLOOR_SYMBOLS, binding.NAVMEM_SYMBOLS, binding.NAVDYN_SYMBOLS, binding.NAVPOSE_SYMBOLS, binding.NAVFOOT_SYMBOLS,
                  binding.NAVSTEER_SYMBOLS, binding.NAVLIVE_SYMBOLS, binding.NAVPATH_SYMBOLS, binding.NAVFRONTIER_SYMBOLS, binding.NAVPLAN_SYMBOLS,
                  binding.NAVCARVE_SYMBOLS, binding.ABI_SYMBOLS):
        assert set(names) <= have
    assert floor_lib.has_navfloor and floor_lib.has_navmem and floor_lib.has_navgrid and floor_lib.backend == "hip-gfx950"
    assert mem - hip_ids(mem) <= have
    extra = have - mem - hip_ids(have)
    assert binding.NAVFLOOR_SYMBOLS == ["ssf_navfloor_default_params", "ssf_navfloor_fit"] and set(binding.NAVFLOOR_SYMBOLS) <= extra
    kernels = extra - set(binding.NAVFLOOR_SYMBOLS)
    assert kernels == {nm for nm in extra if "k_navfloor_" in nm}, sorted(extra)
    for k in ("k_navfloor_prep", "k_navfloor_direction", "k_navfloor_height", "k_navfloor_refine"):
        assert any(k in nm for nm in kernels), k


def test_no_other_library_holds_a_name_of_it(product_lib, oracle_lib):
    for other in [exported(product_lib.path), exported(oracle_lib.path)] + [exported(getattr(binding, nm)) for nm in OLDER]:
        assert not [nm for nm in other if "navfloor" in nm]
    for load in ("load_navcarve", "load_nav", "load_explore", "load_drive", "load_live", "load_steer", "load_foot", "load_pose", "load_dyn", "load_mem"):
        assert not getattr(binding, load)().has_navfloor
    assert not product_lib.has_navfloor and not oracle_lib.has_navfloor


def test_the_products_table_is_the_golden_one(product_lib):
    want = open(os.path.join(ROOT, "tests", "golden", "libssf_hip_dynsyms.txt")).read().split()
    have = sorted(exported(product_lib.path))
    assert have == sorted(want), sorted(set(have) ^ set(want))


def test_an_older_library_names_the_missing_symbol(product_lib):
    lib = binding.load_mem()
    assert not lib.has_navfloor
    f = binding.Fusion.__new__(binding.Fusion)                            # (no handle: the check comes before any call)
    f.L = lib
    with pytest.raises(binding.SsfError, match="ssf_navfloor_fit.*binding.load_floor"):
        f.nav_floor()
    with pytest.raises(binding.SsfError, match="ssf_navfloor_default_params.*binding.load_floor"):
        f.nav_floor_default_params()
    with pytest.raises(binding.SsfError, match="ssf_navfloor_fit.*binding.load_floor"):
        f.nav_floor_grid()


def test_the_symbols_stay_out_of_the_other_headers():
    for nm in binding.NAVFLOOR_SYMBOLS:
        assert nm not in binding.ABI_SYMBOLS
        for hdr in sorted(os.listdir(INCLUDE)):
            if hdr.endswith(".h") and hdr != "ssf_navfloor.h":
                assert nm not in open(os.path.join(INCLUDE, hdr)).read(), (nm, hdr)
        assert nm + "(" in open(os.path.join(INCLUDE, "ssf_navfloor.h")).read()
    assert "#define SSF_ABI_VERSION 3" in open(os.path.join(INCLUDE, "ssf.h")).read()


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_the_header_compiles_on_its_own_and_the_binding_has_its_layout(lang, tmp_path):
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    fields = lambda st: ", ".join("(int)offsetof(%s, %s)" % (st[0], nm) for nm, _ in st[1]._fields_)
    structs = (("ssf_navfloor_params", binding.SsfNavFloorParams), ("ssf_navfloor_out", binding.SsfNavFloorOut),
               ("ssf_navfloor_fit_result", binding.SsfNavFloorFitResult))
    body = "".join('    printf("%s %%d", (int)sizeof(%s));\n    { int o[] = {%s}; for (unsigned i = 0; i < sizeof(o) / sizeof(o[0]); i++) printf(" %%d", o[i]); }\n'
                   '    printf("\\n");\n' % (st[0], st[0], fields(st)) for st in structs)
    consts = '    printf("%d %d %d %d %d %d\\n", SSF_NAVFLOOR_OK, SSF_NAVFLOOR_NO_FLOOR, SSF_NAVFLOOR_DEGENERATE, SSF_NAVFLOOR_DIR_BINS, SSF_NAVFLOOR_HEIGHT_BINS, SSF_NAVFLOOR_MAX_ROUNDS);\n'
    src.write_text('#include "ssf_navfloor.h"\n#include <stddef.h>\n#include <stdio.h>\nint main(void) {\n' + body + consts + "    return 0;\n}\n")
    exe = str(tmp_path / "t")
    r = subprocess.run(["gcc" if lang == "c" else "g++", "-Wall", "-Wextra", "-Werror", "-I", INCLUDE, str(src), "-o", exe], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    for (name, st), line in zip(structs, lines):
        got = [int(v) for v in line.split()[1:]]
        assert line.split()[0] == name and got == [C.sizeof(st)] + [getattr(st, nm).offset for nm, _ in st._fields_], (name, line)
    assert [int(v) for v in lines[-1].split()] == [fr.OK, fr.NO_FLOOR, fr.DEGENERATE, fr.DIR_BINS, fr.HEIGHT_BINS, fr.MAX_ROUNDS]
    assert (binding.NAVFLOOR_DIR_BINS, binding.NAVFLOOR_HEIGHT_BINS, binding.NAVFLOOR_MAX_ROUNDS) == (fr.DIR_BINS, fr.HEIGHT_BINS, fr.MAX_ROUNDS)


def test_the_binding_names_what_the_restatement_names():
    hdr = open(os.path.join(INCLUDE, "ssf_navfloor.h")).read()
    for nm, _ in binding.SsfNavFloorParams._fields_ + binding.SsfNavFloorFitResult._fields_:
        assert re.search(r"\b%s\b" % nm, hdr), nm
    named = {nm for nm, _ in binding.SsfNavFloorParams._fields_}
    assert named - {"t_init_min", "t_init_max", "t_last_min", "t_last_max"} | {"t_init", "t_last"} == set(fr.DEFAULTS)
    result = {nm for nm, _ in binding.SsfNavFloorFitResult._fields_} - {"reserved"}
    assert set(fr.INTEGERS) | set(fr.FLOATS) | {"width", "height"} == result
    assert binding.NAVFLOOR_STATUS[fr.OK] == "ok" and binding.NAVFLOOR_STATUS[fr.NO_FLOOR] == "no_floor" and binding.NAVFLOOR_STATUS[fr.DEGENERATE] == "degenerate"


def test_the_solve_header_is_free_of_hip():
    text = open(os.path.join(ROOT, "supersurfel_fusion_amd", "csrc", "ssf_navfloor_solve.hpp")).read()
    assert "hip" not in text.replace("HIP", "").lower() and "#include \"" not in text


def test_the_replay_options_parse():
    from supersurfel_fusion_amd import replay
    base = ["--npz", "frames.npz", "--nav-grid-dir", "grids"]
    a = replay.parse_args(base + ["--nav-grid-fit-floor"])
    assert replay.nav_fit_floor_of(a) == dict(up=None) and replay.library_of(a) == "load_floor"
    a = replay.parse_args(base + ["--nav-grid-fit-floor", "--nav-floor-up", "0", "0", "1", "--nav-live", "--nav-live-memory", "--nav-grid-carve"])
    assert replay.nav_fit_floor_of(a) == dict(up=(0.0, 0.0, 1.0)) and replay.library_of(a) == "load_floor"
    # without the flag: the library each line gave before
    for extra, want in (([], "load_product"), (["--nav-grid-carve"], "load_navcarve"), (["--nav-plan-goal", "1.0", "2.0"], "load_nav"),
                        (["--nav-frontiers"], "load_explore"), (["--nav-plan-goal", "1.0", "2.0", "--nav-plan-waypoints"], "load_drive"),
                        (["--nav-live"], "load_live"), (["--nav-plan-goal", "1.0", "2.0", "--nav-steer"], "load_steer"),
                        (["--nav-live", "--nav-live-memory"], "load_mem")):
        a = replay.parse_args(base + extra)
        assert replay.nav_fit_floor_of(a) is None and replay.library_of(a) == want, (extra, replay.library_of(a))
    for bad in (["--npz", "frames.npz", "--nav-grid-fit-floor"], base + ["--nav-floor-up", "0", "0", "1"],
                base + ["--nav-grid-fit-floor", "--nav-floor-up", "0", "0", "0"], base + ["--nav-grid-fit-floor", "--nav-floor-up", "0", "1"]):
        with pytest.raises(SystemExit):
            replay.parse_args(bad)
    with pytest.raises(ValueError, match="nav_fit_floor needs nav_grid_dir"):
        replay.replay(None, [], nav_fit_floor=dict(up=None))
