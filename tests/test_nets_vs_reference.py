"""The encoder/decoder definitions in slr_sfs_amd.nets against the reference's own classes, on CPU.
The reference networks were constructed from its real option parser with the canonical flag sets
(train_animating_scripts/*.sh), eval mode, their state dicts replaced by the deterministic ones of
tests/nets_fixture.py (BN statistics randomised), and their outputs stored in tests/golden/nets_vs_reference.npz
(tools/make_golden_reference_checks.py).  Here the same state dicts are regenerated and loaded into ours through
load_reference_state_dict."""
import numpy as np
import pytest
import torch

import nets_fixture as NF


@pytest.fixture(scope="module")
def ref(golden_dir):
    return np.load(f"{golden_dir}/nets_vs_reference.npz")


@torch.no_grad()
def _check(ref, case, tol=2e-4):
    from slr_sfs_amd import nets
    _, cls, args, prefix, _, _ = NF.VS_REFERENCE[case]
    keys = [str(k) for k in ref[f"{case}_keys"]]
    sd = {prefix + k: v for k, v in NF.state_dict("vs_reference/" + case, keys, ref[f"{case}_shapes"]).items()}
    mine = getattr(nets, cls)(*args)
    nets.load_reference_state_dict(mine, sd, prefix)
    with nets.cpu_reference():                      # the torch definition of the fused stages, on the CPU
        b = mine.eval()(NF.vs_reference_input(case))
    b = b if isinstance(b, tuple) else (b,)
    assert len(b) == int(ref[f"{case}_nout"])
    for i, rb in enumerate(b):
        ra = torch.from_numpy(ref[f"{case}_out{i}"])
        assert ra.shape == rb.shape, (case, i, ra.shape, rb.shape)
        scale = ra.abs().max().item() + 1e-6
        assert (ra - rb).abs().max().item() <= tol * scale, ((ra - rb).abs().max().item(), scale)


def test_encoder_with_z(ref):
    _check(ref, "encoder_with_z")


def test_decoder_pconv2_with_holes(ref):
    _check(ref, "decoder_holes")                    # a hole + a single-channel zero: mask update / ratio / resampling
    _check(ref, "decoder_all_hole")                 # everything a hole


def test_bg_decoder_and_alpha_nets(ref):
    _check(ref, "net_bg")
    _check(ref, "alpha_encoder")
    _check(ref, "alpha_decoder")
