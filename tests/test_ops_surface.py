"""The public surface of the ``otpose_amd.ops`` package is what ``otpose_amd/ops.py`` exported when it was one module
(tests/golden/ops_surface.json, written by tests/golden/make_golden_ops_surface.py), plus the five shared helpers that
were private names there; the modules import one way, each on its own; ``ops/__init__.py`` only re-exports."""
import ast
import json
import os
import subprocess
import sys

import pytest

from otpose_amd import ops
from tests.conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
import make_golden_ops_surface as G        # noqa: E402

MODULES = ("base", "dcn", "psroi", "conv", "encoder", "prm", "h16", "decode", "poseval", "data", "loss", "detect", "segments")
PKG = os.path.join(ROOT, "otpose_amd", "ops")


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "ops_surface.json")) as f:
        return json.load(f)


def test_exports_are_the_recorded_names_plus_the_five_renamed_helpers(recorded):
    now = G.surface(ops)
    assert sorted(now) == sorted([*recorded["names"], *G.RENAMED.values()])
    assert sorted(recorded["renamed"]) == sorted(G.RENAMED)


def test_kinds_signatures_and_constant_values_are_the_recorded_ones(recorded):
    now = G.surface(ops)
    assert sum(d["kind"] == "constant" and d["value"] is not None for d in recorded["names"].values()) >= 15
    for name, want in recorded["names"].items():
        assert now[name] == want, name
    for old, new in G.RENAMED.items():
        assert now[new] == recorded["renamed"][old], new


def test_old_private_spellings_are_gone():
    for old in G.RENAMED:
        assert not hasattr(ops, old), old
        for mod in MODULES:
            assert not hasattr(getattr(ops, mod), old), (mod, old)


def test_the_package_is_exactly_the_listed_modules():
    found = sorted(f[:-3] for f in os.listdir(PKG) if f.endswith(".py") and f != "__init__.py")
    assert found == sorted(MODULES)


def test_each_module_imports_on_its_own_in_a_fresh_interpreter():
    """One interpreter per module, all started at once (a cycle shows as an ImportError here)."""
    code = "import otpose_amd.ops.{0} as m; assert m.__name__ == 'otpose_amd.ops.{0}'"
    procs = [subprocess.Popen([sys.executable, "-c", code.format(mod)], cwd=ROOT, stderr=subprocess.PIPE, text=True)
             for mod in MODULES]
    for mod, p in zip(MODULES, procs):
        err = p.communicate()[1]
        assert p.returncode == 0, f"import otpose_amd.ops.{mod}:\n{err}"


def test_imports_go_one_way():
    """``base`` imports no sibling; every other module imports siblings only from ``base`` and ``conv``, ``conv`` only from
    ``base``; nothing imports the package itself."""
    for mod in MODULES:
        with open(os.path.join(PKG, mod + ".py")) as f:
            tree = ast.parse(f.read())
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.level == 1:
                assert node.module is not None, f"{mod}.py imports the package itself"
                allowed = () if mod == "base" else ("base",) if mod == "conv" else ("base", "conv")
                assert node.module in allowed, f"{mod}.py imports .{node.module}"
            if isinstance(node, ast.ImportFrom) and node.level == 2:
                assert node.module != "ops" and all(a.name != "ops" for a in node.names), f"{mod}.py imports the package"
            if isinstance(node, ast.ImportFrom) and node.level == 0:
                assert not (node.module or "").startswith("otpose_amd"), f"{mod}.py: absolute import of the package"


def test_init_only_re_exports():
    with open(os.path.join(PKG, "__init__.py")) as f:
        tree = ast.parse(f.read())
    assert isinstance(tree.body[0], ast.Expr) and isinstance(tree.body[0].value, ast.Constant)        # the docstring
    for node in tree.body[1:]:
        assert isinstance(node, ast.ImportFrom) and all(a.name != "*" for a in node.names), ast.dump(node)[:80]
        if node.level == 2:                             # ``ops.hip``, which ops.py had and a GPU test reaches
            assert node.module is None and [a.name for a in node.names] == ["hip"]
        else:
            assert node.level == 1 and node.module in MODULES, ast.dump(node)[:80]
    from otpose_amd import hip
    assert ops.hip is hip
