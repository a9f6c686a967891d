"""The drop-in boundary: every first-party import at the top of the reference's three driver scripts resolves with
`dropin/` first on the path (what `python -m ditreeonlineplanner_amd.run script.py` sets up), the engine-backed names come
from this package, everything the engine does not replace falls through to the reference checkout, and the
`common.map_utils.cc_calls` counter the drivers reset / read is the engine's.

The import blocks, and the reference modules they reach, are recorded in tests/golden/driver_imports.json
(tests/golden/extract_driver_imports.py); the test rebuilds a stand-in checkout from them.  Third-party modules the machine
lacks (minari, gymnasium, gymnasium_robotics, diffusers, playsound, spatialmath, termcolor) are in-memory placeholders, as
in tests/golden/make_golden.py."""
import importlib
import json
import os
import subprocess
import sys
import textwrap

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = ["run_scenarios.py", "run_scenarios_with_lidar_DiTree.py", "run_scenarios_with_lidar_MPPI.py"]
with open(os.path.join(REPO, "tests", "golden", "driver_imports.json")) as f:
    RECORD = json.load(f)

CHILD = r'''
import importlib, importlib.machinery, json, os, sys, types
ref, repo, block = sys.argv[1], sys.argv[2], json.loads(sys.argv[3])
sys.path[:] = [os.path.join(repo, "dropin"), repo, ref] + [p for p in sys.path if p]
os.environ["DITREE_REFERENCE_ROOT"] = ref
os.chdir(ref)

class _Any(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return type(name, (), {"__init__": lambda self, *a, **k: None, "__call__": lambda self, *a, **k: None})
def placeholder(name):
    parts = name.split(".")
    for i in range(1, len(parts) + 1):
        n = ".".join(parts[:i])
        if n not in sys.modules:
            m = _Any(n); m.__path__ = []; m.__spec__ = importlib.machinery.ModuleSpec(n, None)
            sys.modules[n] = m
THIRD = ["minari", "gymnasium", "gymnasium.spaces", "gymnasium_robotics", "diffusers.schedulers.scheduling_ddpm", "playsound",
         "spatialmath.base", "spatialmath.base.transforms3d", "termcolor", "casadi"]
for n in THIRD:
    try:
        importlib.import_module(n)
    except ImportError:
        placeholder(n)

out = {}
for kind, module, names in block:            # the script's top-level import statements, in order
    m = importlib.import_module(module)
    for name in names:
        getattr(m, name)
    out[module] = getattr(m, "__file__", None) or "<placeholder>"
import common.map_utils
common.map_utils.cc_calls = 0
from ditreeonlineplanner_amd.common import map_utils as engine_mu
engine_mu.add_cc_calls(7)
out["__cc_calls__"] = common.map_utils.cc_calls
out["__same_module__"] = common.map_utils is engine_mu
print("RESULT " + json.dumps(out))
'''


@pytest.fixture(scope="module")
def reference_checkout(tmp_path_factory):
    """A stand-in reference checkout: every recorded module at its path, running its recorded top-level imports and
    defining a placeholder for each name imported from it."""
    root = tmp_path_factory.mktemp("reference")
    for mod in RECORD["reference_modules"].values():
        lines = [f"import {m}" if kind == "import" else f"from {m} import {', '.join(names)}" for kind, m, names in mod["imports"]]
        lines += [f"class {name}:\n    pass" for name in mod["names"]]
        path = root / mod["file"]
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text("\n".join(lines) + "\n")
    return str(root)


def _resolve(script, ref):
    block = json.dumps(RECORD["scripts"][script])
    r = subprocess.run([sys.executable, "-c", CHILD, ref, REPO, block], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[7:])


@pytest.mark.parametrize("script", SCRIPTS)
def test_script_import_block_resolves(script, reference_checkout):
    ref = reference_checkout
    res = _resolve(script, ref)
    pkg = os.path.join(REPO, "ditreeonlineplanner_amd")
    # engine-backed names come from this repository ...
    for mod in ("car_env", "train_diffusion_policy", "policies.fm_policy", "policies.uniform_policy", "planners.RRT",
                "common.map_utils", "drone_env", "planners.random_tree"):
        assert mod in res, (mod, sorted(res))
        assert res[mod].startswith(REPO), (mod, res[mod])
    assert res["common.map_utils"].startswith(pkg)
    # ... what the engine does not replace still comes from the reference checkout
    assert res["planners.MPC"].startswith(ref), res["planners.MPC"]
    for mod in ("obstacle_insertion", "plot_logger"):
        if mod in res:
            assert res[mod].startswith(ref), (mod, res[mod])
    if script.endswith("MPPI.py"):
        assert res["MPPI.mppi"].startswith(REPO)
    # the counter the drivers reset and read (run_scenarios.py:338,343) is the engine's
    assert res["__same_module__"] is True and res["__cc_calls__"] == 7


def test_launcher_puts_dropin_first(tmp_path):
    """`python -m ditreeonlineplanner_amd.run script.py` runs the script as __main__ with dropin/ ahead of the script's own
    directory (plain `python script.py` would put the script's directory first and the reference's packages would win)."""
    root = tmp_path / "ref"
    (root / "planners").mkdir(parents=True)
    (root / "planners" / "__init__.py").write_text("")
    (root / "planners" / "RRT.py").write_text("RRT_Planner = 'reference'\n")
    (root / "planners" / "other.py").write_text("X = 'from the checkout'\n")
    (root / "main.py").write_text(textwrap.dedent("""
        import os, sys
        import planners.RRT, planners.other
        print("RRT", planners.RRT.__file__)
        print("OTHER", planners.other.X)
        print("CWD", os.getcwd())
        print("ARGV", sys.argv[1:])
    """))
    r = subprocess.run([sys.executable, "-m", "ditreeonlineplanner_amd.run", str(root / "main.py"), "--flag", "3"],
                       capture_output=True, text=True, cwd=REPO, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    out = dict(ln.split(" ", 1) for ln in r.stdout.strip().splitlines())
    assert out["RRT"].startswith(os.path.join(REPO, "dropin")), out
    assert out["OTHER"] == "from the checkout"
    assert os.path.realpath(out["CWD"]) == os.path.realpath(str(root))
    assert out["ARGV"] == "['--flag', '3']"


def test_engine_names_win_over_a_reference_checkout_on_the_path(tmp_path, monkeypatch):
    """common.map_utils falls through to the USER's reference checkout for names the engine does not provide (forest / PNG
    helpers) -- it must never let the checkout shadow a hot-path name: is_colliding_car / create_local_map / is_colliding_ant /
    is_colliding_maze / cc_calls stay the engine's even when a checkout that defines them is first on the path."""
    import importlib
    ck = tmp_path / "checkout" / "common"
    ck.mkdir(parents=True)
    (ck / "map_utils.py").write_text(
        "cc_calls = -7\n"
        "def is_colliding_car(*a, **k): return 'REFERENCE'\n"
        "def create_local_map(*a, **k): return 'REFERENCE'\n"
        "def is_colliding_ant(*a, **k): return 'REFERENCE'\n"
        "def is_colliding_maze(*a, **k): return 'REFERENCE'\n"
        "def load_forest_png(path): return ('from the checkout', path)\n")
    monkeypatch.setenv("DITREE_REFERENCE_ROOT", str(tmp_path / "checkout"))
    monkeypatch.syspath_prepend(str(tmp_path / "checkout"))
    from ditreeonlineplanner_amd.common import map_utils as mu
    importlib.reload(mu)
    try:
        for name in ("is_colliding_car", "create_local_map", "is_colliding_ant", "is_colliding_maze", "add_cc_calls"):
            fn = getattr(mu, name)
            assert fn.__module__ == "ditreeonlineplanner_amd.common.map_utils", name       # the engine's, not the checkout's
        assert mu.cc_calls == 0
        assert mu.load_forest_png("x.png") == ("from the checkout", "x.png")              # fall-through for everything else
        with pytest.raises(AttributeError):
            mu.no_such_name
    finally:
        monkeypatch.delenv("DITREE_REFERENCE_ROOT")
        importlib.reload(mu)
