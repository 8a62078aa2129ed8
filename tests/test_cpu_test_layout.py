"""The layout of the test tree, checked on the syntax trees of tests/*.py, tests/golden/*.py and scripts/**/*.py:

  * no file imports a test module; shared helpers live in support modules (the modules of tests/ whose names do not start with
    test_), and a helper that a support module defines is written out nowhere else;
  * every name a file takes from a support module exists there (the scripts need a GPU to run: this is their check);
  * the gradient-name tuple is spelled out once, as util.GRAD_NAMES;
  * every support module imports without the built library and without touching a device, so that collection works anywhere."""
import ast
import glob
import importlib
import os
import sys

import util

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
FILES = sorted(glob.glob(os.path.join(TESTS, "*.py")) + glob.glob(os.path.join(TESTS, "golden", "*.py")) +
               glob.glob(os.path.join(ROOT, "scripts", "**", "*.py"), recursive=True))
TREES = {p: ast.parse(open(p).read(), p) for p in FILES}
# (conftest is pytest's; the *_worker files are programs that tests start, not modules that anything imports)
SUPPORT = sorted(m for m in (os.path.basename(p)[:-3] for p in glob.glob(os.path.join(TESTS, "*.py")))
                 if not m.startswith("test_") and m != "conftest" and not m.endswith("_worker"))


def _imports(tree):
    """(module, name or None, alias, statement) of every import in the tree, function-local ones included"""
    for n in ast.walk(tree):
        if isinstance(n, ast.Import):
            for a in n.names:
                yield a.name, None, a.asname or a.name, n
        elif isinstance(n, ast.ImportFrom) and n.level == 0:
            for a in n.names:
                yield n.module, a.name, a.asname or a.name, n


def _where(path, node):
    return "%s:%d" % (os.path.relpath(path, ROOT), node.lineno)


def test_no_file_imports_a_test_module():
    assert len(FILES) > 100 and len(SUPPORT) >= 16, (len(FILES), SUPPORT)
    bad = [_where(p, n) for p, t in TREES.items() for m, _, _, n in _imports(t) if m.split(".")[0].startswith("test_")]
    assert not bad, "imports of test modules: %s" % bad


def _functions(tree):
    """{name: arguments and body (without the docstring) as a string} of the functions a module defines"""
    out = {}
    for n in tree.body:
        if isinstance(n, ast.FunctionDef):
            body = n.body[1:] if isinstance(n.body[0], ast.Expr) and isinstance(getattr(n.body[0], "value", None), ast.Constant) else n.body
            out[n.name] = ast.dump(n.args) + "".join(ast.dump(b) for b in body)
    return out


def test_a_helper_of_a_support_module_is_written_out_nowhere_else():
    """no test module holds a copy of a support module's function, under any name, and no two support modules hold the same one
    (modules may use one name for different things: camera_cases.census and a test's census fixture)"""
    home = {}
    for m in SUPPORT:
        for name, code in _functions(TREES[os.path.join(TESTS, m + ".py")]).items():
            home.setdefault(code, []).append("%s.%s" % (m, name))
    bad = [v for v in home.values() if len(v) > 1]
    for p, t in TREES.items():
        m = os.path.basename(p)[:-3]
        if os.path.dirname(p) == TESTS and m.startswith("test_"):
            bad += [["%s.%s" % (m, n)] + home[code] for n, code in _functions(t).items() if code in home]
    assert not bad, bad


def _rebinds(fn, name):
    """whether function fn has `name` as an argument, assigns it or imports it"""
    a = fn.args
    return name in [x.arg for x in a.args + a.kwonlyargs + a.posonlyargs + [y for y in (a.vararg, a.kwarg) if y]] or any(
        isinstance(n, ast.Name) and isinstance(n.ctx, ast.Store) and n.id == name or
        isinstance(n, (ast.Import, ast.ImportFrom)) and any((x.asname or x.name) == name for x in n.names) for n in ast.walk(fn))


def _attributes(tree, alias, statement):
    """every `alias.attr` in the function that holds the import statement -- for an import at the top, in the module but for the
    functions that rebind alias"""
    scope = next((f for f in ast.walk(tree) if isinstance(f, ast.FunctionDef) and any(n is statement for n in ast.walk(f))), tree)
    todo = list(ast.iter_child_nodes(scope))
    while todo:
        n = todo.pop()
        if scope is tree and isinstance(n, (ast.FunctionDef, ast.Lambda)) and _rebinds(n, alias):
            continue
        if isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id == alias:
            yield n
        todo += list(ast.iter_child_nodes(n))


def test_every_name_taken_from_a_support_module_exists_there():
    mods = {m: importlib.import_module(m) for m in SUPPORT}
    missing, checked = [], 0
    for p, t in TREES.items():
        for m, name, alias, statement in _imports(t):
            if m in mods:
                uses = [(name, statement)] if name is not None else [(n.attr, n) for n in _attributes(t, alias, statement)]
                checked += len(uses)
                missing += ["%s: %s has no %s" % (_where(p, n), m, attr) for attr, n in uses if not hasattr(mods[m], attr)]
    assert not missing, missing
    assert checked > 300, checked


def test_the_gradient_names_are_spelled_out_once():
    bad = [_where(p, n) for p, t in TREES.items() for n in ast.walk(t)
           if isinstance(n, (ast.Tuple, ast.List)) and [getattr(e, "value", None) for e in n.elts] == list(util.GRAD_NAMES)]
    assert len(bad) == 1 and bad[0].startswith("tests/util.py:"), bad


class _NoLibrary:
    """an import hook under which the built library cannot be imported"""
    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] == "diff_gaussian_rasterization":
            raise ImportError("a support module imports the built library at import time: %s" % name)


def test_support_modules_import_without_the_library_and_without_a_device():
    """imported afresh, with the library out of reach; the modules the other tests hold (and their state) are put back afterwards"""
    held = {k: sys.modules.pop(k) for k in list(sys.modules) if k in SUPPORT or k.split(".")[0] == "diff_gaussian_rasterization"}
    device = lambda: "torch" in sys.modules and sys.modules["torch"].cuda.is_initialized()  # noqa: E731
    before, hook = device(), _NoLibrary()
    sys.meta_path.insert(0, hook)
    try:
        for m in SUPPORT:
            importlib.import_module(m)
        assert device() == before, "importing a support module initialised the device"
    finally:
        sys.meta_path.remove(hook)
        for m in SUPPORT:
            sys.modules.pop(m, None)
        sys.modules.update(held)
