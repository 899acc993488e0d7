"""The decoder's narrow end on the tail route (nets.DecoderPconv2: slr_pconv3x3_forward_tail + slr_narrow_gather for blocks 6 / 7) against
the two-kernel path behind the validation switch nets.staged_narrow_end().

Bound: E = max|frame - ref64| / max|ref64| with ref64 the torch definition of the decoder in float64 (nets.cpu_reference()).  The split-f16
model of a WHOLE decoder is its evaluation on the split kernels that existed before the route -- the two-kernel path -- so that run stands in
for E_model in the project's bound:  E_tail <= 2 E_two_kernel + 10 E_plain32,  E_plain32 the same definition in float32 on the CPU."""
import copy

import pytest
import torch

import split_model as sm

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def S():
    import slr_sfs_amd
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    slr_sfs_amd._lib.lib()
    return slr_sfs_amd


def test_default_route_against_the_validation_switch(S):
    from slr_sfs_amd import nets
    torch.manual_seed(11)
    dec = nets.DecoderPconv2(64, 3).eval()
    with torch.no_grad():
        for m in dec.modules():
            if hasattr(m, "stored_mean"):
                m.stored_mean.normal_(0, 0.3)
                m.stored_var.uniform_(0.5, 1.5)
        x = torch.randn(2, 64, 32, 64)
        x = x * (torch.rand(2, 1, 32, 64) > 0.1)                     # 10 % zero pixels: the derived mask of the first block
        with nets.cpu_reference():
            y32 = dec(x)
            y64 = copy.deepcopy(dec).double()(x.double())
        dec = dec.cuda()
        xd = x.cuda()
        names = []
        call = nets._lib.call
        nets._lib.call = lambda name, *a: (names.append(name), call(name, *a))[1]
        try:
            nets.saturation_count(DEV)
            y_tail, m_tail = dec(xd, return_mask=True)
            tail_names, names = names, []
            with nets.staged_narrow_end():
                y_two, m_two = dec(xd, return_mask=True)
            sat = nets.saturation_count(DEV)
        finally:
            nets._lib.call = call
    assert "slr_pconv3x3_forward_tail" in tail_names and "slr_narrow_gather" in tail_names and "slr_pconv3x3_forward_skipout" not in tail_names
    assert "slr_pconv3x3_forward_tail" not in names and "slr_pconv3x3_forward_skipout" in names
    launches = lambda ns: [n for n in ns if "weights" not in n and "saturation" not in n]      # (the first pass also prepares the weights)
    assert len(launches(tail_names)) == len(launches(names))         # tail + gather in the place of the wide kernel + the <= 4-channel kernel
    assert sat == 0
    assert torch.equal(m_tail, m_two)
    e_tail, e_two, e_plain = sm.E(y_tail, y64), sm.E(y_two, y64), sm.E(y32, y64)
    bound = 2 * e_two + 10 * e_plain
    print(f"decoder 2x64x32x64: E_tail {e_tail:.2e} E_two_kernel {e_two:.2e} E_plain32 {e_plain:.2e} bound {bound:.2e} ratio {e_tail / bound:.3f}; "
          f"tail against two-kernel {sm.E(y_tail, y_two):.2e}")
    assert e_tail <= bound, (e_tail, bound)
