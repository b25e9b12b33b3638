"""The one capture rule (``training._captured_step``) driven with counting fakes, no GPU: two eager steps, one capture
behind the second, replays from then on; SRWN_MODEL_GRAPHS=0 and a failed capture keep the steps eager; a state made for
another sampler starts again at zero.  The routine synchronises the device around a capture: that call is substituted."""
import pytest
import torch

from tests._pkg import sub


class Fakes:
    """An eager step, a capture and a replay that count their calls and say in which order they came."""

    def __init__(self, broken=False):
        self.calls, self.broken = [], broken

    def eager(self):
        self.calls.append("eager")
        return "eager result"

    def capture(self):
        self.calls.append("capture")
        if self.broken:
            raise RuntimeError("no graph today")
        return "the graph"

    def replay(self, captured):
        assert captured == "the graph"
        self.calls.append("replay")
        return "replay result"


class Engine:
    pass


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)
    monkeypatch.delenv("SRWN_MODEL_GRAPHS", raising=False)


def _run(st, f, steps):
    T = sub("training")
    return [T._captured_step(st, "graph", f.eager, f.capture, f.replay) for _ in range(steps)]


def test_two_eager_steps_one_capture_then_replays():
    T, eng, f = sub("training"), Engine(), Fakes()
    st = T._sampler_state(eng, "_eval_state", "sampler", "graph")
    assert st == {"sampler": "sampler", "eager": 0, "graph": None, "failed": False} and eng._eval_state is st
    assert _run(st, f, 1) == ["eager result"] and f.calls == ["eager"] and st["graph"] is None
    assert _run(st, f, 1) == ["eager result"] and f.calls == ["eager", "eager", "capture"] and st["graph"] == "the graph"
    assert _run(st, f, 3) == ["replay result"] * 3
    assert f.calls == ["eager", "eager", "capture", "replay", "replay", "replay"]
    assert st["eager"] == 2 and not st["failed"]


def test_the_capture_is_synchronised_and_collected_first(monkeypatch):
    import gc
    T, f = sub("training"), Fakes()
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: f.calls.append("synchronize"))
    monkeypatch.setattr(gc, "collect", lambda: f.calls.append("collect"))
    _run(T._sampler_state(Engine(), "_fit_state", "sampler", "graph"), f, 3)
    assert f.calls == ["eager", "eager", "synchronize", "collect", "capture", "synchronize", "replay"]


def test_model_graphs_0_never_captures(monkeypatch):
    monkeypatch.setenv("SRWN_MODEL_GRAPHS", "0")
    T, f = sub("training"), Fakes()
    st = T._sampler_state(Engine(), "_fit_state", "sampler", "graph")
    assert _run(st, f, 5) == ["eager result"] * 5
    assert f.calls == ["eager"] * 5 and st["graph"] is None and not st["failed"]


def test_a_failed_capture_is_reported_once_and_not_tried_again(capsys):
    T, f = sub("training"), Fakes(broken=True)
    st = T._sampler_state(Engine(), "_fit_state", "sampler", "graph")
    assert _run(st, f, 5) == ["eager result"] * 5
    assert f.calls == ["eager", "eager", "capture", "eager", "eager", "eager"]
    assert st["graph"] is None and st["failed"]
    assert capsys.readouterr().out == "hipGraph capture failed (no graph today); continuing with eager launches\n"


def test_another_sampler_starts_again_at_zero():
    T, eng, f = sub("training"), Engine(), Fakes()
    first, second = object(), object()
    st = T._sampler_state(eng, "_fit_state", first, "graph")
    _run(st, f, 3)
    assert T._sampler_state(eng, "_fit_state", first, "graph") is st and st["graph"] == "the graph"
    st2 = T._sampler_state(eng, "_fit_state", second, "graph")
    assert st2 is not st and eng._fit_state is st2
    assert st2 == {"sampler": second, "eager": 0, "graph": None, "failed": False}
    del f.calls[:]
    _run(st2, f, 3)
    assert f.calls == ["eager", "eager", "capture", "replay"]
    eng._fit_state = None                                   # (what OptControls.drop_graphs leaves)
    assert T._sampler_state(eng, "_fit_state", second, "graph")["eager"] == 0


def test_train_step_keeps_its_state_on_the_engine():
    """``_train_step``: ``_graph_ready`` / ``_eager_steps`` / ``_graph_failed`` on the engine; after ``drop_graphs`` has
    cleared ``_graph_ready`` the count stays, so one eager step precedes the next capture."""
    T = sub("training")

    class Eng:
        calls = []

        def train_step(self):
            self.calls.append("eager")
            return "loss"

        def capture_graphs(self):
            self.calls.append("capture")

        def train_step_graphed(self):
            self.calls.append("replay")
            return "loss"

    eng = Eng()
    assert [T._train_step(eng) for _ in range(4)] == ["loss"] * 4
    assert eng.calls == ["eager", "eager", "capture", "replay", "replay"] and eng._graph_ready is True
    eng._graph_ready = False
    del eng.calls[:]
    T._train_step(eng), T._train_step(eng)
    assert eng.calls == ["eager", "capture", "replay"] and eng._graph_ready is True and eng._eager_steps == 3
