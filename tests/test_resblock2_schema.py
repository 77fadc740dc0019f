"""ResBlock2 generators (reference models.py:251, modules.py:232-256) on the host side: the checkpoint schema against the
reference's own state_dict key list (recorded as data in tests/golden/resblock2.npz by make_golden_resblock2.py), the
synthetic weights, the ResBlock1 schema left as it was, and the shim's constructor no longer refusing resblock "2".
No GPU: the engine is a recorder."""
import os

import numpy as np
import pytest
import torch

from vispeech_amd import config as vcfg
from vispeech_amd.schema import ModelDims, dims_from_ctor, state_dict_schema, used_by_infer
from vispeech_amd.synth import synth_state_dict


def rb2_args():
    hp = vcfg.default_hparams()
    hp.model["resblock"] = "2"
    return vcfg.synthesizer_args(hp)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "resblock2.npz"))


def test_schema_equals_the_reference_key_list_and_shapes(golden):
    args, kwargs = rb2_args()
    dims = dims_from_ctor(*args, **kwargs)
    assert dims.resblock_kind == 2
    schema = state_dict_schema(dims)
    keys = [str(k) for k in golden["ref_keys"]]
    assert len(keys) == 609 and list(schema) == keys
    for k, row in zip(keys, golden["ref_shapes"]):
        assert tuple(schema[k]) == tuple(int(x) for x in row if x >= 0), k
    rb = [k for k in keys if k.startswith("dec.resblocks.")]
    assert len(rb) == 4 * 3 * 2 * 3 and all(".convs." in k for k in rb)
    assert all(used_by_infer(k) for k in rb)


def test_synthetic_weights_cover_every_resblock2_key():
    args, kwargs = rb2_args()
    dims = dims_from_ctor(*args, **kwargs)
    schema = state_dict_schema(dims)
    sd = synth_state_dict(dims, seed=5)
    assert list(sd) == list(schema)
    assert all(sd[k].shape == tuple(schema[k]) and sd[k].dtype == np.float32 for k in schema)
    inf = synth_state_dict(dims, seed=5, infer_only=True)
    assert {k for k in inf if k.startswith("dec.resblocks.")} == {k for k in schema if k.startswith("dec.resblocks.")}


def test_resblock1_schema_is_unchanged():
    schema = state_dict_schema(ModelDims())
    assert len(schema) == 753
    assert ModelDims().resblock_kind == 1
    assert not any(".convs." in k for k in schema)
    # the shim's divergence from the reference: an int 1 is ResBlock1 here
    args, kwargs = vcfg.synthesizer_args(vcfg.default_hparams())
    assert dims_from_ctor(*args, **dict(kwargs, resblock=1)).resblock_kind == 1


class _RecordingEngine:
    def __init__(self, dims, device="cuda:0"):
        self.dims, self.device, self.ready, self.loaded = dims, torch.device(device), False, None

    def set_weights(self, state_dict, strict=True):
        self.loaded = dict(state_dict)
        return [], []

    def finalize(self):
        self.ready = True


@pytest.mark.parametrize("resblock", ["2", 2, "ResBlock2"])
def test_the_shim_builds_resblock2_models(monkeypatch, resblock):
    import vispeech_amd.models as vm
    monkeypatch.setattr(vm, "Engine", _RecordingEngine)
    args, kwargs = vcfg.synthesizer_args(vcfg.default_hparams())
    kwargs["resblock"] = resblock                         # the reference's test is `resblock == '1'`: anything else is 2
    net = vm.SynthesizerTrn(*args, **kwargs).eval()
    assert net.dims.resblock_kind == 2
    sd = net.state_dict()
    assert len(sd) == 609 and "dec.resblocks.0.convs.1.weight_v" in sd
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth_state_dict(net.dims, seed=3).items()})
    assert net._engine.ready and "dec.resblocks.11.convs.0.weight_g" in net._engine.loaded
