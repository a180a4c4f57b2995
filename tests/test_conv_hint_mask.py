"""A 3x3 conv that carries hint bits of the halo family (emo_gemm_params.tile bits 3, 4, 5: csrc/gemm.hip plan_halo) but is not served by
it - stride 2, or split-K - falls through to the dense path, which must not read those bits as a tile id (bit 3 = 8 forced the 128x128
tile) or as the tile-order override (tile >> 4): the plan is the one of the same conv without them.  Asked of the library on the host."""
import pytest
import torch

from emote_hack_amd import ops

CONVS = [dict(M=2 * 16 * 16, N=320, Cin=128, H=32, stride=2, split_k=1),        # stride 2: the im2col loader
         dict(M=24 * 8 * 8, N=1280, Cin=1280, H=8, stride=1, split_k=8)]        # split-K: not the halo kernel's


def plan(c, dtype, tile):
    Ho = (c["H"] + 2 - 3) // c["stride"] + 1
    return ops.gemm_plan(dtype=dtype, M=c["M"], N=c["N"], K=9 * c["Cin"], bias=True, split_k=c["split_k"], tile=tile,
                         conv=dict(H=c["H"], W=c["H"], Cin=c["Cin"], stride=c["stride"], upsample2x=False, Ho=Ho, Wo=Ho))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("case", range(len(CONVS)))
def test_halo_hint_bits_do_not_reach_the_dense_plan(dtype, case):
    c = CONVS[case]
    base = plan(c, dtype, 0)
    assert base[0] != 1 and base[3] & 1, base                  # not the halo family; the conv loader
    for bits in (8, 16, 32, 8 | 16 | 32):
        assert plan(c, dtype, bits) == base, (bits, plan(c, dtype, bits), base)
        assert plan(c, dtype, 1 | bits) == plan(c, dtype, 1), bits   # the tile pin in bits 0-2 stays
