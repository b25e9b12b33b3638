"""The model module's surface against tests/golden/model_surface.json (tests/golden/make_model_surface.py), recorded
before ``model.py`` was split into ``training.py``, ``model.py`` and ``serving.py``: every class and function it held is
still an attribute of the module, every class with the same methods, signatures, properties and public bases.  Names may
be added.  No GPU: the modules import without one, in any order."""
import json
import os
import subprocess
import sys

import pytest

from tests._pkg import PKG, ROOT, sub
from tests.golden.make_model_surface import describe

with open(os.path.join(ROOT, "tests", "golden", "model_surface.json")) as f:
    GOLDEN = json.load(f)


def test_the_golden_holds_what_it_should():
    assert len(GOLDEN["classes"]) + len(GOLDEN["functions"]) == 72
    assert {"WaveNet", "WaveNetTeacher", "WaveNetAutoEncoder", "ParallelWaveNet", "SiameseWaveNet"} <= set(GOLDEN["classes"])


@pytest.mark.parametrize("name", GOLDEN["functions"])
def test_function_is_still_there(name):
    assert callable(getattr(sub("model"), name))


@pytest.mark.parametrize("name", sorted(GOLDEN["classes"]))
def test_class_keeps_its_shape(name):
    want, got = GOLDEN["classes"][name], describe(getattr(sub("model"), name))
    assert got["bases"] == want["bases"]
    assert set(want["properties"]) <= set(got["properties"])
    for method, signature in want["methods"].items():
        assert got["methods"].get(method) == signature, "%s.%s" % (name, method)


@pytest.mark.parametrize("order", ["model training serving", "training serving model", "serving model training"])
def test_the_three_modules_import_in_any_order(order):
    code = "import importlib\nfor m in %r.split():\n    importlib.import_module(%r + m)\n" % (order, PKG.__name__ + ".")
    subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True)
