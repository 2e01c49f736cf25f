"""`ResidualBlock(..., skip=b)` off the HIP bf16 path: the block concatenates
and runs exactly as it does on a pre-concatenated input."""
import torch

from flaxdiff_amd import ops
from flaxdiff_amd.models import ResidualBlock, Unet


def _grads(rb, fn, tensors):
    for p in rb.parameters():
        p.grad = None
    ts = [t.clone().requires_grad_(True) for t in tensors]
    y = fn(*ts)
    y.square().mean().backward()
    return y.detach(), [t.grad for t in ts], \
        {n: p.grad.clone() for n, p in rb.named_parameters()}


def test_skip_equals_preconcatenated_input_on_cpu():
    torch.manual_seed(3)
    rb = ResidualBlock("conv", 64 + 64, 64, temb_features=16, norm_groups=8)
    x, b = torch.randn(2, 8, 8, 64), torch.randn(2, 8, 8, 64)
    temb = torch.randn(2, 16)
    y1, (gx1, gb1), gp1 = _grads(rb, lambda x_, b_: rb(x_, temb, skip=b_), [x, b])
    y2, (gc2,), gp2 = _grads(
        rb, lambda c_: rb(c_, temb), [torch.cat([x, b], -1)])
    assert torch.equal(y1, y2)
    assert torch.equal(torch.cat([gx1, gb1], -1), gc2)
    for n in gp1:
        assert torch.equal(gp1[n], gp2[n]), n


def test_ineligible_inputs_take_the_concat_route(monkeypatch):
    """CPU tensors, and channel counts that are no multiple of 64, never reach
    the two-source Function."""
    def boom(*a, **k):
        raise AssertionError("group_norm_cat_dense called for ineligible input")
    monkeypatch.setattr(ops, "group_norm_cat_dense", boom)
    calls = []
    real_cat = ops.cat_channels
    monkeypatch.setattr(ops, "cat_channels",
                        lambda a, b: calls.append(1) or real_cat(a, b))
    torch.manual_seed(4)
    rb = ResidualBlock("conv", 8 + 16, 16, temb_features=16, norm_groups=4)
    x, b = torch.randn(2, 4, 4, 8), torch.randn(2, 4, 4, 16)
    temb = torch.randn(2, 16)
    y = rb(x, temb, skip=b)
    assert calls == [1]
    assert torch.equal(y, rb(torch.cat([x, b], -1), temb))
    gamma, w = rb.norm1.weight, rb.residual_conv.weight
    assert not ops.virtual_cat_eligible(x, b, 4, gamma, rb.norm1.bias, w,
                                        rb.residual_conv.bias)


def test_knob_switches_the_route_off(monkeypatch):
    monkeypatch.setenv("FD_VIRTUAL_CAT", "0")
    assert not ops.virtual_cat_enabled()
    monkeypatch.setenv("FD_VIRTUAL_CAT", "1")
    assert ops.virtual_cat_enabled()
    monkeypatch.delenv("FD_VIRTUAL_CAT")
    assert ops.virtual_cat_enabled()


def test_unet_state_dict_keys_unchanged():
    model = Unet(emb_features=32, feature_depths=[16, 32],
                 attention_configs=[None, None], num_res_blocks=1,
                 num_middle_res_blocks=1, norm_groups=4)
    keys = set(model.state_dict().keys())
    # digest of the sorted key list of this configuration before the skip
    # argument existed
    import hashlib
    assert len(keys) == 95
    assert hashlib.sha256("\n".join(sorted(keys)).encode()).hexdigest() == \
        "2f4fdd6c3aa2db83a431ec056a3099f0b9168fd8b5da5bddc2e5104cd37aaf0a"
    # the decoder blocks own the same parameters as any ResidualBlock; nothing
    # is registered for the skip route
    assert not any("skip" in k or "cat" in k for k in keys)
    rb = model.up_blocks[0]["res"][0]
    assert {n for n, _ in rb.named_parameters()} == {
        "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias",
        "conv1.weight", "conv1.bias", "temb_projection.weight",
        "temb_projection.bias", "conv2.weight", "conv2.bias",
        "residual_conv.weight", "residual_conv.bias"}
    # forward still runs end to end on CPU through the concat route
    x = torch.randn(1, 8, 8, 3)
    y = model(x, torch.rand(1), None)
    assert y.shape == (1, 8, 8, 3)
