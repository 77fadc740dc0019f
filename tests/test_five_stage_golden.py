"""Five-stage generators (upsample_rates [8, 8, 2, 2, 2], 512 initial channels: stages of 256, 128, 64, 32 and 16
channels) on the host side: the checkpoint schema against the real reference's own state_dict key list, and the CPU
oracle against the real reference's outputs, both recorded as data in tests/golden/five_stage.npz by
make_golden_five_stage.py.  This pins the oracle for five stages; the GPU tests of tests/test_five_stage_model.py rest on
the same fixture."""
import os

import numpy as np
import pytest
import torch

from oracle.vispeech_oracle import Oracle, generator
from vispeech_amd import config as vcfg
from vispeech_amd.schema import dims_from_ctor, state_dict_schema
from vispeech_amd.synth import synth_state_dict

FIVE_STAGE = dict(upsample_rates=[8, 8, 2, 2, 2], upsample_kernel_sizes=[16, 16, 4, 4, 4], upsample_initial_channel=512)


def five_stage_dims(resblock="1"):
    hp = vcfg.default_hparams()
    for k, v in FIVE_STAGE.items():
        hp.model[k] = v
    hp.model["resblock"] = resblock
    args, kwargs = vcfg.synthesizer_args(hp)
    return dims_from_ctor(*args, **kwargs)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "five_stage.npz"))


@pytest.mark.parametrize("resblock,prefix,n_keys", [("1", "", 810), ("2", "rb2_", 630)])
def test_schema_equals_the_reference_key_list_and_shapes(g, resblock, prefix, n_keys):
    dims = five_stage_dims(resblock)
    assert dims.total_upsample == 512
    assert [dims.upsample_initial_channel >> (i + 1) for i in range(5)] == [256, 128, 64, 32, 16]
    schema = state_dict_schema(dims)
    keys = [str(k) for k in g[prefix + "ref_keys"]]
    assert len(keys) == n_keys and list(schema) == keys
    for k, row in zip(keys, g[prefix + "ref_shapes"]):
        assert tuple(schema[k]) == tuple(int(x) for x in row if x >= 0), k
    assert tuple(schema["dec.conv_post.weight"]) == (1, 16, 7)


def test_oracle_infer_matches_the_reference(g):
    dims = five_stage_dims("1")
    orc = Oracle(synth_state_dict(dims, seed=int(g["weight_seed"])), dims)
    out = orc.infer(g["in_phonemes"], g["in_lengths"], g["in_sid"], noise=g["noise"], noise_scale=0.667,
                    duration_control=g["in_duration"], pitch_control=g["in_f0"], energy_control=g["in_energy"])
    np.testing.assert_array_equal(out["x_mask"].numpy(), g["x_mask"])
    assert g["x_mask"].sum(axis=(1, 2)).astype(int).tolist() == [26, 13, 30]
    for name in ("m_p", "logs_p", "z_p", "z"):
        e = rel_err(out[name].numpy(), g[name])
        assert e <= 1e-5, (name, e)
    assert out["o"].shape == (3, 1, 30 * 512)
    assert rel_err(out["o"].numpy(), g["o"]) <= 1e-4


@pytest.mark.parametrize("resblock,key", [("1", "o"), ("2", "rb2_o")])
def test_oracle_generator_matches_the_reference_waveform(g, resblock, key):
    """The fp64 oracle's generator on the golden's z * x_mask, for both ResBlock kinds."""
    dims = five_stage_dims(resblock)
    w = Oracle(synth_state_dict(dims, seed=int(g["weight_seed"])), dims, dtype=torch.float64).w
    gv = w["emb_g.weight"][torch.from_numpy(g["in_sid"])][:, :, None]
    z = torch.from_numpy(g["z"]).double() * torch.from_numpy(g["x_mask"]).double()
    with torch.no_grad():
        wave = generator(w, z, gv, dims)
    assert rel_err(wave.numpy(), g[key]) <= 1e-4
