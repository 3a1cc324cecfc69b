"""The Python surface of the engines, pinned: `physicsvae_amd.engine` is split by job over five modules (its docstring
names them), and nothing a caller could import or call changed with the split.

`golden/engine_surface.json` was written by running this file as a script on the commit before the split (`surface()` below:
the signature of every public callable of `physicsvae_amd.engine`, its public data names, and every public method and
property of the five classes).  The tests: the tree gives that list again -- nothing missing, nothing changed (new names
may come); both engines take every PPO method from the one class in `engine_ppo`; and each new module imports alone."""
import ast
import inspect
import json
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_surface.json")
CLASSES = ("HipEngine", "StackSetEngine", "Stack", "Arch", "GraphedInfer")
PPO_METHODS = ("ppo_bind", "ppo_reset", "ppo_step", "ppo_sgd", "ppo_launches", "ppo_grad_step", "ppo_apply",
               "ppo_peer_export", "ppo_peer_open", "ppo_peer_close", "ppo_peer_status", "ppo_evaluate", "ppo_prepare",
               "ppo_act", "gae_launches")
NEW_MODULES = ("arch", "engine_ppo", "engine_dp", "engine_rollout", "stack_set", "engine")


def surface():
    from physicsvae_amd import _lib
    from physicsvae_amd import engine as E
    out = {}
    for name in sorted(n for n in dir(E) if not n.startswith("_")):
        v = getattr(E, name)
        if inspect.ismodule(v) or getattr(_lib, name, None) is v:     # (modules and `_lib`'s constants: imports, not surface)
            continue
        out[name] = str(inspect.signature(v)) if callable(v) else "data: %s" % type(v).__name__
    for cls in CLASSES:
        c = getattr(E, cls)
        for name in sorted(n for n in dir(c) if not n.startswith("_") or n in ("__init__", "__call__", "__getitem__", "__iter__")):
            v = inspect.getattr_static(c, name)
            if isinstance(v, property):
                out["%s.%s" % (cls, name)] = "property"
            elif isinstance(v, (classmethod, staticmethod)):
                out["%s.%s" % (cls, name)] = "%s%s" % (type(v).__name__, inspect.signature(v.__func__))
            elif inspect.isfunction(v):
                out["%s.%s" % (cls, name)] = str(inspect.signature(v))
    return out


def test_surface_is_the_parents():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = surface()
    assert len(want) > 100                      # (the list is the whole surface, not a stub)
    missing = sorted(set(want) - set(got))
    changed = {n: (want[n], got[n]) for n in want if n in got and got[n] != want[n]}
    assert not missing and not changed, (missing, changed)


def is_shim(cls, fn):
    """A signature shim: after its docstring the body is ONE statement of at most two source lines, `return
    self._ppo_<body>(...)`, and that `_ppo_<body>` is the shared class's.  Anything else (a second statement, another
    callee, an override of the callee) is a second body."""
    from physicsvae_amd.engine_ppo import PpoSurface
    body = ast.parse(textwrap.dedent(inspect.getsource(fn))).body[0].body
    if body and isinstance(body[0], ast.Expr) and isinstance(body[0].value, ast.Constant):
        body = body[1:]
    if len(body) != 1 or not isinstance(body[0], ast.Return) or not isinstance(body[0].value, ast.Call):
        return False
    f = body[0].value.func
    if not (isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name) and f.value.id == "self" and f.attr.startswith("_ppo_")):
        return False
    return body[0].end_lineno - body[0].lineno + 1 <= 2 and inspect.getattr_static(cls, f.attr) is PpoSurface.__dict__.get(f.attr)


@pytest.mark.parametrize("cls", ("HipEngine", "StackSetEngine"))
def test_one_ppo_surface(cls):
    from physicsvae_amd import engine as E
    from physicsvae_amd import engine_ppo
    c = getattr(E, cls)
    assert issubclass(c, engine_ppo.PpoSurface)
    for name in PPO_METHODS:
        fn = getattr(c, name)
        if inspect.getmodule(fn) is engine_ppo:
            assert fn is getattr(engine_ppo.PpoSurface, name)
        else:
            assert is_shim(c, fn), "%s.%s is neither the shared method nor a signature shim over its body" % (cls, name)
    for name in ("_need_gpu", "_stream", "_ppo"):
        assert inspect.getattr_static(c, name) is engine_ppo.PpoSurface.__dict__[name]


@pytest.mark.parametrize("module", NEW_MODULES)
def test_module_imports_alone(module):
    """Each module imports in a fresh interpreter (no cycle).  `arch`, `engine_ppo`, `engine_dp` and `engine_rollout` stand
    on `_lib` and torch alone: importing one of them loads none of the other five."""
    others = [m for m in NEW_MODULES if m != module] if module in NEW_MODULES[:4] else []
    code = ("import sys, physicsvae_amd.%s\n"
            "bad = [m for m in %r if 'physicsvae_amd.' + m in sys.modules]\n"
            "assert not bad, bad\n" % (module, others))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    json.dump(surface(), sys.stdout, indent=1, sort_keys=True)
    print()
