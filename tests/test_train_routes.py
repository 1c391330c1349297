"""`otpose_amd.train_ops.TrainRoutes`: the training step's `OTPOSE_*` switches, read once per forward.  Every name keeps its
spelling, default and meaning; nothing else in the training modules reads the environment; one Winograd rule for both engines."""
import dataclasses
import os
import re

import pytest

import otpose_amd
from otpose_amd import ops
from otpose_amd.engine import InferenceEngine
from otpose_amd.train_ops import TrainRoutes

# switch -> (field, default, a non-default setting, the field's value under it)
SWITCHES = {
    "OTPOSE_TRAIN_STREAMS": ("train_streams", True, "0", False),
    "OTPOSE_TRAIN_RECOMPUTE": ("recompute", True, "0", False),
    "OTPOSE_PACK_BATCH": ("pack_batch", True, "0", False),
    "OTPOSE_BLOCK_FUSE": ("block_fuse", True, "0", False),
    "OTPOSE_BF16_OFFSETS": ("bf16_offsets", True, "0", False),
    "OTPOSE_BF16_MLP": ("bf16_mlp", True, "0", False),
    "OTPOSE_MLP_FUSED_TRAIN": ("mlp_fused_train", False, "1", True),
    "OTPOSE_DENSE_CC": ("use_dense_cc", True, "0", False),
    "OTPOSE_CONV_MATH": ("use_x3", True, "f32", False),
    "OTPOSE_WINOGRAD": ("use_winograd", True, "0", False),
    "OTPOSE_WGRAD_STREAM": ("wgrad_stream", True, "0", False),
}


@pytest.fixture
def clean_env(monkeypatch):
    for name in [k for k in os.environ if k.startswith("OTPOSE_")]:
        monkeypatch.delenv(name)
    return monkeypatch


def test_every_field_has_its_switch_and_default(clean_env):
    r = TrainRoutes.from_env()
    assert {f.name for f in dataclasses.fields(TrainRoutes)} == {field for field, *_ in SWITCHES.values()}
    for name, (field, default, _, _) in SWITCHES.items():
        assert getattr(r, field) == default and type(getattr(r, field)) is type(default), name
    assert r == TrainRoutes()


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_a_switch_flips_its_own_field_and_no_other(clean_env, name):
    field, _, setting, value = SWITCHES[name]
    base = dataclasses.asdict(TrainRoutes.from_env())
    clean_env.setenv(name, setting)
    assert dataclasses.asdict(TrainRoutes.from_env()) == {**base, field: value}


@pytest.mark.parametrize("setting", ["0", "", "2", "true"])
def test_the_fused_training_mlp_is_opt_in(clean_env, setting):
    clean_env.setenv("OTPOSE_MLP_FUSED_TRAIN", setting)
    assert TrainRoutes.from_env().mlp_fused_train is False


def test_routes_are_frozen():
    with pytest.raises(dataclasses.FrozenInstanceError):
        TrainRoutes().use_winograd = False


def test_the_training_modules_read_the_environment_only_in_from_env():
    pkg = os.path.dirname(otpose_amd.__file__)
    for mod in ("train.py", "train_ops.py", "bf16_ops.py"):
        inside, stray = False, []
        for no, line in enumerate(open(os.path.join(pkg, mod)), 1):
            if re.match(r"\s*(def|class) ", line):                  # from_env's body runs to the next def / class
                inside = mod == "train_ops.py" and line.strip().startswith("def from_env(")
            if re.search(r"os\.environ|getenv", line) and not inside:
                stray.append((no, line.strip()))
        assert not stray, (mod, stray)


@pytest.mark.parametrize("cin,cout,pays", [(64, 64, True), (48, 48, True), (32, 48, True), (48, 32, False), (24, 48, False),
                                           (32, 64, False)])     # 64 outputs would compute two 48-row tiles: 96 > 1.15 * 64 = 73.6
def test_winograd_pays_is_one_rule(cin, cout, pays):
    assert ops.winograd_pays(cin, cout) is pays
    assert InferenceEngine.winograd_pays is ops.winograd_pays
