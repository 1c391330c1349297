#!/usr/bin/env python
"""Generate tests/golden/ops_surface.json: the public surface of ``otpose_amd.ops`` (needs no GPU and no reference).

Run from the repo root:  ``python tests/golden/make_golden_ops_surface.py``

The committed file was recorded at the last commit at which ``otpose_amd/ops.py`` was one module; tests/test_ops_surface.py
holds the ``otpose_amd.ops`` package to it.  Recorded for every public name (no leading underscore; imported modules, the
``__future__`` feature and classes / functions of other distributions are not part of the surface): its kind - ``function``
(any callable that is not a class), ``class`` or ``constant`` -, for a callable ``str(inspect.signature(...))`` (``null`` where
Python cannot tell, e.g. ``Function.apply``), for a constant its value with tuples written as lists (``null`` when it is not
plain numbers / strings).  ``renamed``: the five helpers that were private names of ops.py and are public names of the
package, recorded under their old spelling from whichever spelling the tree has, so that the recipe writes the same file on
either side of the split."""
from __future__ import annotations

import inspect
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

RENAMED = {"_require_gpu": "require_gpu", "_check_f32": "check_f32", "_out_hw": "out_hw", "_joints_mse": "joints_mse",
           "_rel_pe_table": "rel_pe_table"}


def plain(value):
    """``value`` as JSON writes it when it is numbers / strings in tuples / lists / dicts, else ``None``."""
    if isinstance(value, (bool, int, float, str)):
        return value
    if isinstance(value, (tuple, list)):
        items = [plain(v) for v in value]
        return None if any(v is None for v in items) else items
    if isinstance(value, dict):
        items = {str(k): plain(v) for k, v in value.items()}
        return None if any(v is None for v in items.values()) else items
    return None


def describe(obj):
    if not callable(obj):
        return {"kind": "constant", "value": plain(obj)}
    try:
        sig = str(inspect.signature(obj))
    except (TypeError, ValueError):
        sig = None
    return {"kind": "class" if inspect.isclass(obj) else "function", "signature": sig}


def is_surface(name, obj):
    if name.startswith("_") or isinstance(obj, types.ModuleType) or type(obj).__module__ == "__future__":
        return False
    if inspect.isclass(obj) or inspect.isfunction(obj):
        return obj.__module__.split(".")[0] == "otpose_amd"
    return True


def surface(ops):
    """{name: description} of the public names of the module / package ``ops``."""
    return {name: describe(obj) for name, obj in sorted(vars(ops).items()) if is_surface(name, obj)}


def main():
    from otpose_amd import ops
    renamed = {old: describe(getattr(ops, old, None) or getattr(ops, new)) for old, new in RENAMED.items()}
    names = {n: d for n, d in surface(ops).items() if n not in RENAMED.values()}
    path = os.path.join(HERE, "ops_surface.json")
    with open(path, "w") as f:
        json.dump({"names": names, "renamed": renamed}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{path}: {len(names)} names, {len(renamed)} renamed")


if __name__ == "__main__":
    main()
