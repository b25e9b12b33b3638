"""Generates tests/golden/model_surface.json: what ``sr-wavenet_amd/model.py`` offers by name.

Run from the repo root: ``python tests/golden/make_model_surface.py`` (no GPU needed: it only imports the module).

For every class and function the model module defines itself or takes from its two halves (``training``, ``serving``):
the name; for a class also the signature of every method found on it (inherited, static and class methods included),
which of its attributes are properties, and its public base classes in order.  tests/test_model_surface.py holds the
module to it: names may be added, none may go or change shape.
"""
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from tests._pkg import PKG, sub  # noqa: E402

HOMES = tuple("%s.%s" % (PKG.__name__, m) for m in ("model", "training", "serving"))


def describe(cls):
    """{"bases": [...], "properties": [...], "methods": {name: signature}} of `cls`, what it inherits included (a method
    may move to a base and back; what a caller finds on the class may not change)."""
    methods, props = {}, []
    for name in sorted(dir(cls)):
        if hasattr(object, name):
            continue
        v = inspect.getattr_static(cls, name)
        if isinstance(v, property):
            props.append(name)
        elif isinstance(v, (staticmethod, classmethod)):
            methods[name] = str(inspect.signature(v.__func__))
        elif inspect.isfunction(v):
            methods[name] = str(inspect.signature(v))
    return {"bases": [b.__name__ for b in cls.__bases__ if b is not object and not b.__name__.startswith("_")],
            "properties": props, "methods": methods}


def surface(module):
    out = {"classes": {}, "functions": []}
    for name, v in sorted(vars(module).items()):
        if getattr(v, "__module__", None) not in HOMES:
            continue
        if inspect.isclass(v):
            out["classes"][name] = describe(v)
        elif inspect.isfunction(v):
            out["functions"].append(name)      # (private helpers: their callers are all in the package)
    return out


if __name__ == "__main__":
    s = surface(sub("model"))
    with open(os.path.join(HERE, "model_surface.json"), "w") as f:
        json.dump(s, f, indent=0, sort_keys=True)
        f.write("\n")
    print("%d names, %d methods" % (len(s["classes"]) + len(s["functions"]),
                                    sum(len(c["methods"]) for c in s["classes"].values())))
