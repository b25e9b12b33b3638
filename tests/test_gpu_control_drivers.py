"""GPU test of the drivers' training-control flags: ``examples/classifier.py --device-data`` under ``--lr-schedule``,
``--clip``, ``--ema``, ``--validate-ema`` and ``--resume``, stopped after 4 steps and started again to 8, prints the losses
and validation lines of one run of 8 steps.  (The driver's ``main(argv)`` is called in this process: three runs cost what
one process start would.)"""
import importlib.util
import os
import re

import pytest

from tests._pkg import ROOT

pytestmark = pytest.mark.gpu


def _run(capsys, logdir, steps, *flags):
    spec = importlib.util.spec_from_file_location("classifier_driver", os.path.join(ROOT, "examples", "classifier.py"))
    drv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(drv)
    capsys.readouterr()
    drv.main(["--train", "--device-data", "--steps", str(steps), "--num-samples", "256", "--layers", "3", "--batch-size", "2",
              "--print-steps", "2", "--device-clips", "6", "--validation-clips", "5", "--validate-every", "2",
              "--eval-batch-size", "4", "--seed", "0", "--logdir", str(logdir), "--lr-schedule", "piecewise:1,5:3e-3,1e-3,3e-4",
              "--clip", "0.5", "--ema", "0.9", "--validate-ema"] + list(flags))
    return re.findall(r"^Step: +(\d+) \| (Loss: [0-9.]+|Validation: .*)$", capsys.readouterr().out, flags=re.M)


def test_classifier_driver_resumes_under_controls(tmp_path, capsys):
    whole = _run(capsys, tmp_path / "whole", 8, "--resume")
    assert len(whole) == 8 and os.path.exists(tmp_path / "whole" / "train_state")
    first = _run(capsys, tmp_path / "parts", 4, "--resume")
    second = _run(capsys, tmp_path / "parts", 8, "--resume")
    assert first == whole[:4]
    assert second == whole[4:]
    assert not os.path.exists(tmp_path / "whole" / "train_state-3.pt") and os.path.exists(tmp_path / "parts" / "train_state-3.pt")
