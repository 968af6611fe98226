"""joint_tensorf_amd/mesh_ops.py: the shared argument checks answer in the name of the entry point that was called, `ops` still
offers every mesh name, and the module stands without `ops`.  No GPU needed: every call here is refused before a launch."""
import ast
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every mesh name tests/ and tools/ reach as ops.X, written out by hand
REACHED_THROUGH_OPS = (
    "COMPONENTS_MAX_SWEEPS", "COMPONENTS_TILE", "RASTER_STATUS", "cap_lattice", "compact_mesh", "component_sizes", "grow_triangles",
    "keep_components", "last_components_stats", "lattice_components", "mesh_count", "mesh_emit", "mesh_from_lattice", "mesh_offsets",
    "ndc_to_world", "raster_draw", "raster_project", "raster_resolve", "raster_resolve_texture", "rasterize", "select_triangles",
    "simplify_cells", "simplify_clusters", "simplify_compact", "simplify_index", "simplify_keys", "simplify_mesh", "simplify_segments",
    "simplify_triangles", "texture_layout", "texture_pack", "texture_texels", "triangle_visibility", "visible_fold", "visible_options",
    "visible_tally", "visible_triangles")


def _bad_calls():
    """(entry point, a call with vertices [4, 2], a call with int64 triangles); for the three that take no such pair the nearest
    two refusals they have"""
    from joint_tensorf_amd import mesh_ops
    V, T, N, P = torch.zeros(4, 3), torch.zeros(2, 3, dtype=torch.int32), torch.zeros(4, 3), torch.zeros(2, 3, 4)
    status, keep = torch.zeros(4, dtype=torch.uint8), torch.ones(2, dtype=torch.uint8)
    lo, hi = (0, 0, 0), (1, 1, 1)
    layout = mesh_ops.texture_layout(2, 4)
    both = {
        "compact_mesh": lambda v, t: (v, t, status),
        "simplify_mesh": lambda v, t: (v, t, N, lo, hi, 2),
        "texture_texels": lambda v, t: (v, t, N, layout),
        "rasterize": lambda v, t: (v, t, P, 8, 8),
        "triangle_visibility": lambda v, t: (v, t, P, 8, 8),
        "select_triangles": lambda v, t: (v, t, keep),
    }
    calls = [(name, args(V[:, :2], T), args(V, T.long())) for name, args in both.items()]
    calls.append(("grow_triangles", (T[:, :2], 4, keep, 1), (T.long(), 4, keep, 1)))
    calls.append(("mesh_from_lattice", (torch.zeros(4, 4), 0.5, lo, hi), (torch.zeros(4, 4, 4), 0.5, (0, 0), hi)))
    calls.append(("ndc_to_world", (V[:, :2], 1.0, 1.0, 1.0), (V, 1.0, 1.0, 1.0, N[:3])))
    return calls


def test_a_refusal_names_the_entry_point_that_was_called():
    from joint_tensorf_amd import mesh_ops
    calls = _bad_calls()
    assert len(calls) == 9
    for name, *bad in calls:
        for args in bad:
            with pytest.raises(ValueError) as e:
                getattr(mesh_ops, name)(*args)
            assert str(e.value).startswith(name + ": "), (name, str(e.value))


def test_ops_keeps_every_mesh_name():
    from joint_tensorf_amd import mesh_ops, ops
    assert len(set(mesh_ops.__all__)) == len(mesh_ops.__all__)
    for name in mesh_ops.__all__:
        assert getattr(ops, name) is getattr(mesh_ops, name), name
    assert sorted(set(REACHED_THROUGH_OPS) - set(mesh_ops.__all__)) == []
    assert ops._stream is mesh_ops._stream


def test_mesh_ops_stands_without_ops():
    """imported first in a fresh interpreter; and no import statement of the module names `ops`"""
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import joint_tensorf_amd.mesh_ops as m; "
                        "print(len(m.__all__))" % ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and int(r.stdout.split()[-1]) > 0, r.stderr[-2000:]
    tree = ast.parse(open(os.path.join(ROOT, "joint_tensorf_amd", "mesh_ops.py")).read())
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom):
            assert node.module != "ops" and all(a.name != "ops" for a in node.names), ast.dump(node)
        if isinstance(node, ast.Import):
            assert all(not a.name.endswith("ops") for a in node.names), ast.dump(node)
