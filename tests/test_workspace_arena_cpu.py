"""CPU: the workspace arena of tests/test_gpu_workspace_contract.py on host tensors, and the completeness of that module's case table
against the code: every engine wrapper that takes its workspace from `_workspace` (or `MeshDB.workspace`) has a case, and every size
function of include/mp_engine.h is reached by a case or excluded by name with a reason.  A wrapper added without a case fails here,
before anyone needs a GPU."""
import ast
import re
from pathlib import Path

import pytest
import torch

import test_gpu_workspace_contract as contract
from support import workspace_arena as wa

ROOT = Path(__file__).resolve().parent.parent


# ---- the arena ---------------------------------------------------------------------------------------------------------------------------
def test_slices_have_the_length_of_engine_workspace_and_start_256_aligned():
    a = wa.WorkspaceArena(1 << 16)
    for n, want in ((0, 256), (1, 256), (255, 256), (256, 256), (257, 257), (4097, 4097)):
        ws = a.workspace(n, "cpu")
        assert ws.dtype == torch.uint8 and ws.numel() == want == max(n, 256) and ws.data_ptr() % 256 == 0 and ws.is_contiguous()
    assert a.slice(17).numel() == 17                       # what MeshDB's slot gets: exactly the reported size
    assert [n for _, n in a.handouts] == [256, 256, 256, 256, 257, 4097, 17]


def test_handouts_are_disjoint_each_between_its_own_canaries():
    a = wa.WorkspaceArena(1 << 16)
    one, two = a.workspace(300), a.workspace(1000)
    (o1, n1), (o2, n2) = a.handouts
    assert o1 - wa.HEAD >= 0 and o1 + n1 + wa.TAIL <= o2 - wa.HEAD, "a hand-out overlaps the canaries of the one before"
    assert one.data_ptr() + n1 + wa.TAIL + wa.HEAD <= two.data_ptr()
    for off, n in a.handouts:
        assert (a.buf[off - wa.HEAD:off] == wa.CANARY).all() and (a.buf[off + n:off + n + wa.TAIL] == wa.CANARY).all()
    one.fill_(1)
    two.fill_(2)                                           # the whole of both slices: no canary is inside one
    a.check()
    with pytest.raises(AssertionError):
        a.workspace(1 << 16)                               # the arena never grows: the same hand-outs land on the same bytes


def test_fills_set_the_workspace_bytes_and_leave_the_canaries():
    a = wa.WorkspaceArena(1 << 14)
    ws = a.workspace(1000)
    for byte in (0x00, 0xFF, 0x5A):
        a.fill(byte)
        assert (ws == byte).all()
        a.check()
    a.fill_random(7)
    first = ws.clone()
    a.check()
    assert 200 < len(set(first.tolist())) and not (first == first[0]).all()
    a.fill_random(7)
    assert torch.equal(ws, first), "the random fill is seeded"
    a.fill_random(8)
    assert not torch.equal(ws, first)
    a.reset()
    a.fill(0xFF)
    assert (a.workspace(1000) == 0xFF).all(), "a fill before the hand-out is what the launch finds"


@pytest.mark.parametrize("n", [256, 1000, 4097])
def test_a_single_damaged_byte_is_reported_with_its_offset_from_the_workspace_end(n):
    a = wa.WorkspaceArena(1 << 15)
    a.workspace(512)
    a.workspace(n)
    off, length = a.handouts[1]
    assert length == n
    a.check()
    for pos, offset in ((off + n, 0), (off - 1, -(n + 1)), (off + n + wa.TAIL - 1, wa.TAIL - 1), (off - wa.HEAD, -(n + wa.HEAD))):
        old = int(a.buf[pos])
        a.buf[pos] = 0x00
        with pytest.raises(wa.CanaryDamage) as e:
            a.check()
        assert (e.value.handout, e.value.length, e.value.offset, e.value.value) == (1, n, offset, 0), str(e.value)
        assert f"offset {offset} from the workspace's end" in str(e.value)
        a.buf[pos] = old
        a.check()
    a.buf[off + n + 5] = 1
    a.buf[off + n + 3] = 2                                  # the FIRST damaged byte
    assert a.damage().offset == 3 and a.damage().value == 2
    a.buf[a.handouts[0][0] - 2] = 9                         # an earlier hand-out is reported before a later one
    assert (a.damage().handout, a.damage().offset) == (0, -(512 + 2))


def test_keep_hands_out_the_same_bytes_unmodified():
    a = wa.WorkspaceArena(1 << 15)
    a.fill_random(3)
    ws = a.workspace(700)
    ws[:] = torch.arange(700, dtype=torch.int64).to(torch.uint8)
    left, ptr = ws.clone(), ws.data_ptr()
    a.keep()
    assert a.handouts == []
    again = a.workspace(700)
    assert again.data_ptr() == ptr and torch.equal(again, left)
    a.check()
    # a smaller launch after a larger one finds the larger one's bytes, and its own canaries inside them
    a.keep()
    small = a.workspace(300)
    assert small.data_ptr() == ptr and torch.equal(small, left[:300]) and (a.buf[a.handouts[0][0] + 300:a.handouts[0][0] + 300 + wa.TAIL] == wa.CANARY).all()


# ---- the table against the code --------------------------------------------------------------------------------------------------------
def _functions(tree):
    """name -> FunctionDef of engine.py's functions; a method as Class.name"""
    out = {}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef):
            out[node.name] = node
        elif isinstance(node, ast.ClassDef):
            for m in node.body:
                if isinstance(m, ast.FunctionDef):
                    out[f"{node.name}.{m.name}"] = m
    return out


def _calls(fn):
    """(names called as plain functions, (receiver, attribute) of the calls through an attribute, every mp_*_bytes attribute named)"""
    names, attrs, sizes = set(), set(), set()
    for node in ast.walk(fn):
        if isinstance(node, ast.Call):
            if isinstance(node.func, ast.Name):
                names.add(node.func.id)
            elif isinstance(node.func, ast.Attribute) and isinstance(node.func.value, ast.Name):
                attrs.add((node.func.value.id, node.func.attr))
        if isinstance(node, ast.Attribute) and re.fullmatch(r"mp_\w+_(workspace|scratch)_bytes\w*", node.attr):
            sizes.add(node.attr)
    return names, attrs, sizes


@pytest.fixture(scope="module")
def engine_graph():
    fns = _functions(ast.parse((ROOT / "megapose6d_amd" / "engine.py").read_text()))
    return fns, {name: _calls(fn) for name, fn in fns.items()}


def _reaches(graph, start, target):
    seen, todo = set(), [start]
    while todo:
        f = todo.pop()
        if f in seen or f not in graph:
            continue
        seen.add(f)
        if target in graph[f][0]:
            return True
        todo += list(graph[f][0])
    return False


def _size_fns_of(graph, start):
    """the size functions an entry names, itself or in the module functions it calls, MeshDB.workspace through `db.workspace` included"""
    seen, todo, out = set(), [start], set()
    while todo:
        f = todo.pop()
        if f in seen or f not in graph:
            continue
        seen.add(f)
        names, attrs, sizes = graph[f]
        out |= sizes
        todo += list(names) + (["MeshDB.workspace"] if ("db", "workspace") in attrs else [])
    return out


HELPERS = {"pose_error_workspace"}     # hands a workspace on to its caller: not an entry itself


def test_every_wrapper_that_takes_a_workspace_has_a_case(engine_graph):
    fns, graph = engine_graph
    takers = {f for f in graph if "." not in f and not f.startswith("_") and f not in HELPERS and _reaches(graph, f, "_workspace")}
    assert "pose_error_workspace" in graph and _reaches(graph, "pose_error_workspace", "_workspace")
    table = {c["entry"] for c in contract.CASES.values() if c["via"] == "_workspace"}
    assert takers == table, (sorted(takers - table), sorted(table - takers))
    assert "raster_render_scene" in takers and len(takers) >= 22
    # the wrappers on a MeshDB slot: raster_render launches, raster_job_flags reads what the launch left
    on_slot = {f for f, (_, attrs, _) in graph.items() if ("db", "workspace") in attrs}
    assert on_slot == {"raster_render", "raster_job_flags"}
    slot_cases = [c for c in contract.CASES.values() if c["via"] == "MeshDB.workspace"]
    assert {c["entry"] for c in slot_cases} == {"raster_render"} and any(c.get("reads") == "raster_job_flags" for c in slot_cases)
    # nothing else in the module allocates a launch's scratch by hand, except the entries the contract module names as not covered
    # (a byte tensor whose one size argument is a byte count: a *_bytes call, or one of the names the module gives such a count)
    by_hand = {f for f, fn in fns.items() for n in ast.walk(fn) if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute)
               and n.func.attr in ("empty", "zeros") and any(k.arg == "dtype" and "uint8" in ast.dump(k.value) for k in n.keywords)
               and len(n.args) == 1 and re.search(r"_bytes|id='need'", ast.dump(n.args[0]))}
    assert by_hand == {"_workspace", "MeshDB.workspace", "icp_refine", "Backbone.workspace", "DetectorNet.forward"}, by_hand


def test_every_case_names_the_size_functions_its_entry_calls(engine_graph):
    _, graph = engine_graph
    for name, c in contract.CASES.items():
        assert set(c["size_fns"]) == _size_fns_of(graph, c["entry"]), name


def test_every_size_function_of_the_header_is_reached_or_excluded_by_name():
    header = (ROOT / "include" / "mp_engine.h").read_text()
    declared = re.findall(r"size_t (mp_\w+_(?:workspace|scratch)_bytes\w*)\(", header)
    assert len(declared) == len(set(declared)) == len(re.findall(r"size_t mp_\w+_(workspace|scratch)_bytes", header)) >= 24
    reached = {f for c in contract.CASES.values() for f in c["size_fns"]}
    excluded = set(contract.EXCLUDED_SIZE_FNS)
    assert not reached & excluded
    assert set(declared) == reached | excluded, (sorted(set(declared) - reached - excluded), sorted((reached | excluded) - set(declared)))
    assert all(len(reason) > 20 for reason in contract.EXCLUDED_SIZE_FNS.values())


def test_the_table_is_plain_data_with_two_shapes_a_case_and_a_known_launch_for_every_raster_shape():
    assert set(contract._BUILDERS) == {c["entry"] for c in contract.CASES.values()}
    for name, c in contract.CASES.items():
        assert len(c["shapes"]) >= 2 and len(set(c["shapes"])) == len(c["shapes"]) and c["shapes"][0] == "one", name
        assert set(c) <= {"entry", "via", "size_fns", "shapes", "launches", "after", "reads"}
        if c["via"] == "MeshDB.workspace":
            for shape in c["shapes"]:
                own, before = contract.RASTER_LAUNCHES[c["launches"][shape]], contract.RASTER_LAUNCHES[c["after"][shape]]
                # the launch before run E is on the same mesh (the same database and slot) and larger: more views and no smaller a frame
                assert before[0] == own[0] and len(before[1]) > len(own[1]) and before[3] >= own[3] and before[4] >= own[4], (name, shape)
                assert len(own[1]) % own[2] == 0 and len(before[1]) % before[2] == 0
    assert len(contract.ITEMS) == sum(len(c["shapes"]) for c in contract.CASES.values())
    assert all(d[0] in contract.CASES for d in contract.DONORS)
    assert len({contract.CASES[d[0]]["entry"] for d in contract.DONORS}) >= 2, "an entry needs a donor that is not itself"
