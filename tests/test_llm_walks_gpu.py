"""The walks of the LoRA-Llama stack state ONE decoder layer (msr3d_amd/llm/decoder.py::decoder_layer / decoder_stack):
`CachedDecoder.prefill(positions="arange")` and the full forward `LoRALlamaStack.logits` run the same kernels with the
same arguments over the same prompt, so the last position's logits must agree bit for bit -- at one key tile and at two.
The fixture model of tests/generate_helpers.py (2 layers, hidden 512, 8 heads of 64, vocab 1024), B = 2, row 1
left-padded by 5."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def net():
    from tests.generate_helpers import gpu_stack
    return gpu_stack(0)[0]


@pytest.mark.parametrize("T", [64, 128])
def test_prefill_is_the_full_forward_bit_for_bit(net, T):
    from msr3d_amd.llm import CachedDecoder
    from tests.generate_helpers import prompt
    x, mask = prompt(0, B=2, T=T, left_pad=5)
    x, mask = x.cuda().to(torch.bfloat16), mask.cuda()
    with torch.no_grad():
        want = net.logits(x, mask, from_position=T - 1)[:, 0]
    dec = CachedDecoder(net)
    dec.reserve(1, 0)
    got = dec.prefill(x, mask, positions="arange")
    k0, v0 = dec.cache.k(0).clone(), dec.cache.v(0).clone()
    assert got.shape == want.shape == (2, 1024)
    assert torch.equal(got, want)
    again = dec.prefill(x, mask, positions="arange")
    assert torch.equal(again, got)
    assert torch.equal(dec.cache.k(0), k0) and torch.equal(dec.cache.v(0), v0)
    assert float(k0.float().abs().max()) > 0.0
