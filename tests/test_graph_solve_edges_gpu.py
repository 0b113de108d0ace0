"""ssf_graph_solve (include/ssf_graph_solve.h) on the MI355X where test_graph_solve_gpu.py does not go: every ending of the inner
loop, the breakdown's freeze inside a chunk of host reads, the chunk shapes (inner_check of 1, beyond max_inner, beyond the p.q
history), 256 / 257 nodes and constraints, the sorts' third digit pass, a hub node, 64 outer steps, working buffers reused across
problem sizes, and the optional pointers.  The inputs are test_graph_solve.py's EDGE_CASES, proven there on the numpy restatement;
every comparison is at 0 bits."""
import numpy as np
import pytest

import graph_solve_ref as gs
import test_graph_gpu as tg
import test_graph_solve as cpu
import test_graph_solve_gpu as sg
import util
from supersurfel_fusion_amd import binding

pytestmark = pytest.mark.gpu
f32 = np.float32


def built(product_lib, c, room=0):
    """a handle with the case's model set and its graph built; the nodes are the case's own"""
    n = len(c["model"][0]["confidences"])
    f = tg.handle(product_lib, 640, 480, nb_supersurfels_max=max(n, room) + 8192)
    rebuild(f, c)
    return f


def rebuild(f, c):
    f.set_model(c["model"][0], c["model"][1], 500)
    assert f.graph_build(stride=c["stride"], look=c["look"]) == len(c["npos"])
    util.assert_same_bits(f.graph_nodes()[0], c["npos"], "nodes")


def solve_edge_case(f, name):
    c, e = cpu.edge_case(name), cpu.EDGE_CASES[name]
    res, R, t = sg.solve_and_check(f, c["look"], c["src"], c["t_init"], c["dst"], name, ref=cpu.edge_solution(name)[1:], **e["params"])
    assert res["inner_end"] == e["end"], (name, res)                 # the table's ending, not merely the restatement's
    return res, R, t


# ---- 1. every edge case -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cpu.EDGE_CASES))
def test_edge_case_equals_the_restatement(name, product_lib):
    f = built(product_lib, cpu.edge_case(name))
    res, _, _ = solve_edge_case(f, name)
    if name == "check_beyond_max":
        assert len(res["inner"]) == binding.GRAPH_SOLVE_MAX_OUTER == 64


# ---- 2. after a breakdown -----------------------------------------------------------------------------------------------------------
def test_after_a_breakdown_the_handle_is_sound(product_lib):
    c = cpu.edge_case("late_breakdown")
    params = cpu.EDGE_CASES["late_breakdown"]["params"]
    a, b = built(product_lib, c), built(product_lib, c)
    res, R, t = solve_edge_case(a, "late_breakdown")
    # through the frozen launches a second time: the same record, the same bytes
    res1 = a.graph_solve(c["src"], c["t_init"], c["dst"], **params)
    R1, t1 = a.graph_transforms()
    assert res1 == res and R1.tobytes() == R.tobytes() and t1.tobytes() == t.tobytes()
    # the next solve starts clean
    sg.solve_and_check(a, c["look"], c["src"], c["t_init"], c["dst"], "defaults after the breakdown")
    # and the breakdown solve's transforms bend the map as the same transforms uploaded do
    assert a.graph_solve(c["src"], c["t_init"], c["dst"], **params) == res
    a.graph_apply_solved()
    b.graph_apply(R, t)
    util.compare_state(a, b, maps=False, frame_surfels=False)
    before = np.ascontiguousarray(c["model"][0]["positions"], f32).reshape(-1, 3)
    assert (a.get_model()["positions"].reshape(-1, 3) != before).any()


# ---- 3. one handle, problems of different sizes -------------------------------------------------------------------------------------
def test_working_buffers_are_reused_across_problem_sizes(product_lib):
    """the node, constraint and sort groups grow one at a time; a smaller problem afterwards ignores the stale tails"""
    short = cpu.BLOCKS
    small = cpu.loop_case(n=2560, stride=10, look=6, n_con=20)      # m = 256, the first sizes of all three groups
    wide = cpu.edge_case("nc513")                                    # m = 257 fits the node group; constraints and sort items grow
    large = cpu.loop_case(n=6000, stride=10, look=6, n_con=40)      # m = 600: the node group grows, the constraint buffers stay
    assert (len(small["npos"]), len(wide["npos"]), len(large["npos"])) == (256, 257, 600)
    ref = lambda c: gs.solve(c["npos"], c["nt0"], c["look"], c["src"], c["t_init"], c["dst"], **short)
    f = built(product_lib, small, room=6000)
    solve = lambda c, what, r: sg.solve_and_check(f, c["look"], c["src"], c["t_init"], c["dst"], what, ref=r, **short)
    ref_small = ref(small)
    res1, R1, t1 = solve(small, "1 small", ref_small)
    rebuild(f, wide)
    res2, R2, t2 = solve(wide, "2 wide", cpu.edge_solution("nc513")[1:])
    # a refused call in between changes nothing: the argument checks come before anything is touched
    bad = wide["src"].copy(); bad[7, 1] = np.nan
    with pytest.raises(binding.SsfError, match=r"\(-1\)"):
        f.graph_solve(bad, wide["t_init"], wide["dst"], **short)
    Rk, tk = f.graph_transforms()
    assert Rk.tobytes() == R2.tobytes() and tk.tobytes() == t2.tobytes()
    assert f.graph_solve(wide["src"], wide["t_init"], wide["dst"], **short) == res2
    Rk, tk = f.graph_transforms()
    assert Rk.tobytes() == R2.tobytes() and tk.tobytes() == t2.tobytes()
    rebuild(f, large)
    solve(large, "3 large", ref(large))
    rebuild(f, small)
    res4, R4, t4 = solve(small, "4 small again", ref_small)
    assert res4 == res1 and R4.tobytes() == R1.tobytes() and t4.tobytes() == t1.tobytes()


# ---- 4. the optional pointers, through the library itself ------------------------------------------------------------------------------
def test_optional_result_and_transform_pointers(product_lib):
    name = "m257"
    c, e = cpu.edge_case(name), cpu.EDGE_CASES[name]
    _, Rr, tr, _ = cpu.edge_solution(name)
    f = built(product_lib, c)
    L, p, m = product_lib.lib, binding.SsfGraphSolveParams(), len(c["npos"])
    assert L.ssf_graph_solve_default_params(p) == 0
    for k, v in e["params"].items():
        setattr(p, k, v)
    ptr = lambda a: a.ctypes.data
    src, t0, dst = (np.ascontiguousarray(c[k]) for k in ("src", "t_init", "dst"))
    assert L.ssf_graph_solve(f.h, p, ptr(src), ptr(t0), ptr(dst), len(src), None) == 0
    R, t = f.graph_transforms()
    util.assert_same_bits(R, Rr, "rotations of a solve without a result record")
    util.assert_same_bits(t, tr, "translations of a solve without a result record")
    canary = np.uint32(0xDEADBEEF)
    rot, trans = np.full((m + 3, 9), canary, np.uint32), np.full((m + 3, 3), canary, np.uint32)
    assert L.ssf_graph_get_transforms(f.h, ptr(rot), None, m) == 0
    assert rot[:m].tobytes() == Rr.tobytes() and (rot[m:] == canary).all() and (trans == canary).all()
    rot[:] = canary
    assert L.ssf_graph_get_transforms(f.h, None, ptr(trans), m) == 0
    assert trans[:m].tobytes() == tr.tobytes() and (trans[m:] == canary).all() and (rot == canary).all()
    assert L.ssf_graph_get_transforms(f.h, None, None, m) == -1
