"""Shapes of the attention sweeps, shared by tests/test_gpu_attention_sweeps.py (which launches them) and the CPU coverage test in
tests/test_host_logic.py (which asks emo_attention_plan what they would launch).  Plain data, no device needed."""
import torch

DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def head_dims(dtype):
    """Every head dim the ABI admits: d % V == 0 up to 160 (V = 16-byte vector: 4 f32 / 8 two-byte elements)."""
    v = 4 if dtype == torch.float32 else 8
    return list(range(v, 161, v))


ALL_DIMS = [(dt, d) for dt in DTYPES for d in head_dims(dt)]

# a. streaming, two segments: 205 = 3 tiles + 13 keys, 77 = 1 tile + 13 keys; the bank is read by batch row 1 only
STREAM = dict(B=2, heads=3, Lq=150, Lk0=205, Lk1=77, seg1_first_batch=1)
# ... and with B * heads a multiple of 8 (the XCD block orders): seg1_first_batch 2 = reversed order, 0 = forward
STREAM_ORDERED = dict(B=4, heads=4, Lq=150, Lk0=205, Lk1=77)
# b. resident walk: one ragged KV tile; Lq 300 = 3 q tiles (2 per block, the last group holds one), 520 = 5 q tiles (4 per block)
RESIDENT = dict(B=20, heads=8, Lk0=50)
RESIDENT_LQ = {300: 2, 520: 4}          # Lq -> q tiles per block the launch rule gives at 160 (b, head) chunks
RESIDENT_DIV = (1, 4)
# c. causal
CAUSAL = dict(B=2, heads=3)
CAUSAL_L = (77, 200)
CAUSAL_RESIDENT = dict(B=20, heads=8, L=150)   # resident wherever the three tiles fit the ring
# d. key-count / query-count edges
EDGE_DIMS = (24, 40, 160)
EDGE_LK = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129)
EDGE_LQ = (1, 33, 129)
EDGE = dict(B=2, heads=2, Lk0_front=128)
# e. ring schedule matrix: (dtype, d) per ring depth in play
RING = [(torch.bfloat16, 40), (torch.float16, 40), (torch.bfloat16, 160), (torch.float16, 160), (torch.float32, 40), (torch.float32, 160)]
RING_TILES0 = (1, 2, 3, 4, 5)
RING_TILES1 = (0, 1, 2, 3, 4)


def plan(dtype, d, *, B, Lq, Lk0, heads, Lk1=0, causal=False):
    from emote_hack_amd import ops
    return ops.attention_plan(dtype=dtype, B=B, Lq=Lq, Lk0=Lk0, heads=heads, d=d, Lk1=Lk1, causal=causal)


def streaming_shapes(d):
    """(kwargs of plan()) of every sweep launch that must take the streaming kernel at head dim d."""
    s, so = STREAM, STREAM_ORDERED
    out = [dict(B=s["B"], Lq=s["Lq"], Lk0=s["Lk0"], heads=s["heads"], Lk1=s["Lk1"]),
           dict(B=so["B"], Lq=so["Lq"], Lk0=so["Lk0"], heads=so["heads"], Lk1=so["Lk1"])]
    out += [dict(B=CAUSAL["B"], Lq=L, Lk0=L, heads=CAUSAL["heads"], causal=True) for L in CAUSAL_L]
    return out


def resident_shapes(d):
    return [dict(B=RESIDENT["B"], Lq=Lq, Lk0=RESIDENT["Lk0"], heads=RESIDENT["heads"]) for Lq in RESIDENT_LQ]
