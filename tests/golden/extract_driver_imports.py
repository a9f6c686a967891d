"""Record the top-level import blocks of the reference's three driver scripts as data (tests/test_dropin_imports.py).

For every script: its module-level `import` / `from ... import` statements, in order.  For every module the reference
checkout ships as a file and those statements reach (directly, or through such a module's own top-level imports): the
file's path in the checkout, the names imported from it and its own top-level imports.  The test rebuilds a stand-in
checkout from this and resolves the import blocks against `dropin/`.  Writes tests/golden/driver_imports.json.

    python tests/golden/extract_driver_imports.py /path/to/DiTreeOnlinePlanner"""
import ast
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SCRIPTS = ["run_scenarios.py", "run_scenarios_with_lidar_DiTree.py", "run_scenarios_with_lidar_MPPI.py"]


def import_block(path):
    block = []
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.Import):
            block += [["import", a.name, []] for a in node.names]
        elif isinstance(node, ast.ImportFrom) and node.level == 0:
            block.append(["from", node.module, [a.name for a in node.names]])
    return block


def main(ref):
    scripts = {script: import_block(os.path.join(ref, script)) for script in SCRIPTS}
    shipped, todo = {}, [st for block in scripts.values() for st in block]
    while todo:
        _, module, names = todo.pop(0)
        rel = module.replace(".", "/") + ".py"
        if not os.path.isfile(os.path.join(ref, rel)):
            continue
        if module not in shipped:
            shipped[module] = {"file": rel, "names": [], "imports": import_block(os.path.join(ref, rel))}
            todo += shipped[module]["imports"]
        entry = shipped[module]
        entry["names"] += [n for n in names if n not in entry["names"]]
    with open(os.path.join(HERE, "driver_imports.json"), "w") as f:
        json.dump({"scripts": scripts, "reference_modules": dict(sorted(shipped.items()))}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
