"""Host tests of the GIF reader: the numpy reference of tests/gif_decode_ref.py against Pillow on every case of
tests/gif_decode_cases.py, byte for byte - so that the GPU tests can hold the kernels against the reference -, what the cases claim
about themselves, parse_gif's fields and refusals, the rate rule of read_video, and what the entries refuse without a device."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from emote_hack_amd import ops
from emote_hack_amd import video_io as V
from emote_hack_amd._lib import EmoHipError
from tests import gif_decode_cases as K
from tests import gif_decode_ref as R


def one_frame_file(h, w, cs, data):
    """a file of one whole frame around image data, with a global table of 1 << cs entries (at least 4: code size 2 serves 2 and 4)"""
    table = K.palette(max(1 << cs, 4), cs)
    return R.build(w, h, [R.frame(np.zeros((h, w), np.uint8), code_size=cs, data=data)], table), table


def parsed_frames(data):
    """a file through parse_gif, the reference LZW decoder and the descriptor-level reference: what decode_gif computes, on the host"""
    p = V.parse_gif(data)
    indices = []
    for f in p.frames:
        got, st = R.lzw_decode(f.data, f.code_size, f.width * f.height)
        assert st == R.OK
        indices.append(got)
    frames, status = R.compose_descriptors(indices, V.gif_descriptors(p.frames, {}), p.tables, p.height, p.width)
    assert status == [R.OK] * len(p.frames)
    return frames


# ------------------------------------------------------------------------------------------------------------------------------ the cases
def test_stream_cases_are_what_they_claim():
    s = K.valid_streams()
    for name, (indices, cs, data, rec) in s.items():
        got, st = R.lzw_decode(data, cs, indices.size)
        assert st == R.OK and got == indices.tobytes(), name
    flat = s["flat"][3]
    assert flat["max_len"] > 64 and flat["kwkwk"] == flat["codes"] - 4           # all but Clear, the first literal, the tail and End of Information
    assert s["noise_clear"][3]["full"] and s["noise_deferred"][3]["full"] and s["deferred_waves"][3]["full"]
    assert s["noise_deferred"][3]["codes"] > 3838 + 1000                         # many codes behind the full table
    assert s["noise_clear"][2] != R.lzw_encode(s["noise_clear"][0], 8, clear_when_full=False)
    assert s["cs2"][3]["max_len"] > 4 and all(s[f"cs{c}"][3]["codes"] > (1 << (c + 1)) for c in (2, 3, 5, 7))      # the width grows from c + 1 bits
    assert len(s["too_many"][2]) > len(R.lzw_encode(s["too_many"][0], 7)) + 300
    no_clear, double = s["no_leading_clear"], s["double_clear"]
    assert no_clear[2] != R.lzw_encode(no_clear[0], 8) and len(double[2]) > len(R.lzw_encode(double[0], 8))
    assert R.lzw_decode(s["no_eoi"][2], 6, s["no_eoi"][0].size + 1)[1] == R.PAST_END


@pytest.mark.parametrize("name", sorted(K.valid_streams()))
def test_reference_decoder_equals_pillow_on_stream_cases(name):
    indices, cs, data, _ = K.valid_streams()[name]
    h, w = indices.shape
    file, table = one_frame_file(h, w, cs, data)
    want = R.pillow_frames(file)
    assert want.shape == (1, h, w, 3) and np.array_equal(want[0], table[indices])
    assert np.array_equal(parsed_frames(file), want)


def test_damaged_streams_are_what_they_claim_and_pillow_raises_on_the_cut_ones():
    d = K.damaged_streams()
    for name, (n, cs, data, status, produced, got_status, got) in d.items():
        assert got_status == status, name
    assert d["short_with_eoi"][4] == 17 * 45 and 0 < d["cut_without_eoi"][4] < 31 * 45 and d["empty"][4] == 0
    assert d["above_next_free"][4] == 2 and d["above_clear_behind_clear"][4] == 2 and d["above_clear_at_start"][4] == 0
    for name, (h, w) in (("short_with_eoi", (31, 45)), ("cut_without_eoi", (31, 45)), ("empty", (31, 45)), ("cut_noise", (64, 96))):
        file, _ = one_frame_file(h, w, 8, d[name][2])
        with pytest.raises(OSError):
            R.pillow_frames(file)


@pytest.mark.parametrize("name", K.BUILT)
def test_reference_composition_equals_pillow_on_built_files(name):
    data, W, H, frames, table, background = K.built(name)
    want = R.pillow_frames(data)
    assert want.shape == (len(frames), H, W, 3)
    assert np.array_equal(R.compose(W, H, frames, table, background), want)
    assert np.array_equal(parsed_frames(data), want)


def test_reference_composition_equals_pillow_on_the_random_batch():
    seen = set()
    for seed in K.RANDOM_SEEDS:
        data, W, H, frames, table, background = K.random_file(seed)
        want = R.pillow_frames(data)
        assert np.array_equal(R.compose(W, H, frames, table, background), want), seed
        assert np.array_equal(parsed_frames(data), want), seed
        for f in frames:
            seen.add((f["disposal"] if f["control"] else None, f["transparent"] is not None, f["table"] is not None, f["interlace"]))
    assert len(K.RANDOM_SEEDS) >= 60
    assert {s[0] for s in seen} == {None, 0, 1, 2, 3} and len(seen) > 30          # the batch reaches the combinations


@pytest.mark.parametrize("name", sorted(K.pillow_files()))
def test_parsed_files_of_pillow_compose_to_what_pillow_reads(name):
    data = K.pillow_files()[name]
    assert np.array_equal(parsed_frames(data), R.pillow_frames(data))


def test_pillow_files_hold_what_they_are_for():
    p = {k: V.parse_gif(v) for k, v in K.pillow_files().items()}
    for d in range(1, 4):
        assert {f.disposal for f in p[f"disposal{d}"].frames} == {d}
    assert any((f.width, f.height) != (56, 40) for f in p["disposal1"].frames)   # Pillow crops the frames to what changed
    assert p["interlaced"].frames[0].interlace and p["two_colours"].frames[0].interlace      # (Pillow interlaces stills only)
    assert all(f.transparent == 0 for f in p["transparency"].frames) and all(f.transparent == 3 for f in p["transparency_keep"].frames)
    assert p["two_colours"].frames[0].table_entries <= 4 and len(p["two_colours_clip"].frames) == 3
    assert p["photos"].loop == 2 and p["disposal0"].loop == 0 and p["optimized"].loop is None
    assert [f.delay for f in p["photos"].frames] == [Fraction(3, 100), Fraction(4, 100), Fraction(3, 100), Fraction(3, 100)]


def test_own_writer_layout_composes_to_palette_of_indices():
    for name, (data, indices, palettes, delays, loop) in K.own_writer_files().items():
        p = V.parse_gif(data)
        want = np.stack([palettes[k if len(palettes) > 1 else 0][indices[k]] for k in range(len(indices))])
        assert np.array_equal(parsed_frames(data), want) and np.array_equal(R.pillow_frames(data), want), name
        assert [f.delay * 100 for f in p.frames] == delays and p.loop == loop and V.gif_fps(p.delays) == 30
        assert all(f.disposal == 1 and f.transparent is None and f.code_size == 8 and f.table_entries == 256 for f in p.frames)
    p = V.parse_gif(K.own_writer_files()["frame_strips8"][0])
    assert [f.table_row for f in p.frames] == [1, 2, 3] and p.tables.shape == (4, 256, 3) and np.array_equal(p.tables[0], p.tables[1])


# ------------------------------------------------------------------------------------------------------------------------------ parse_gif
def test_parse_gif_fields():
    g = K.palette(16)
    frames = [R.frame(K.noise(5, 6, 16, 1), 1, 2, delay=7, disposal=0),
              R.frame(K.noise(3, 3, 4, 2), 4, 0, table=K.palette(4, 5), transparent=2, disposal=3, delay=12),
              R.frame(K.noise(2, 2, 16, 3), 0, 0, control=False),
              R.frame(K.noise(8, 9, 16, 4), 0, 0, disposal=0, delay=0, control=True, interlace=True),
              R.frame(K.noise(1, 1, 8, 5), 8, 7, table=K.palette(8, 6), disposal=2, delay=65535, transparent=5),
              R.frame(K.noise(2, 3, 16, 6), 0, 0, transparent=15, delay=1)]
    p = V.parse_gif(R.build(9, 8, frames, g, background=9, loop=7, comment=b"x" * 300))
    assert (p.version, p.width, p.height, p.background, p.global_entries, p.loop, p.trailer) == (b"GIF89a", 9, 8, 9, 16, 7, True)
    assert [(f.left, f.top, f.width, f.height) for f in p.frames] == [(1, 2, 6, 5), (4, 0, 3, 3), (0, 0, 2, 2), (0, 0, 9, 8), (8, 7, 1, 1), (0, 0, 3, 2)]
    assert p.delays == (Fraction(7, 100), Fraction(12, 100), Fraction(0), Fraction(0), Fraction(65535, 100), Fraction(1, 100))
    assert [f.transparent for f in p.frames] == [None, 2, None, None, 5, 15]
    assert [f.disposal_bits for f in p.frames] == [0, 3, 0, 0, 2, 0]
    assert [f.disposal for f in p.frames] == [0, 3, 3, 3, 2, 2]                   # sticky: bits 0 and a missing extension inherit
    assert [f.fill for f in p.frames] == [9, 2, 9, 9, 5, 15]                   # transparent, else the background 
    assert [f.table_row for f in p.frames] == [0, 1, 0, 0, 2, 0] and [f.table_entries for f in p.frames] == [16, 4, 16, 16, 8, 16]
    assert [f.interlace for f in p.frames] == [False, False, False, True, False, False] and [f.code_size for f in p.frames] == [4, 2, 4, 4, 3, 4]
    assert p.tables.shape == (3, 256, 3) and np.array_equal(p.tables[0, :16], g) and not p.tables[0, 16:].any() and not p.tables[1, 4:].any()
    big = R.frame(K.noise(40, 50, 256, 7))
    data = R.build(50, 40, [big], K.palette(256, 1))
    q = V.parse_gif(data)
    assert q.frames[0].data == R.lzw_encode(big["indices"], 8) and len(q.frames[0].data) > 255 and q.loop is None     # sub-blocks joined
    assert V.parse_gif(data[:-1]).trailer is False and V.parse_gif(data[:-1]).frames == q.frames
    no_global = V.parse_gif(R.build(4, 4, [R.frame(K.noise(4, 4, 4, 1), table=K.palette(4))], None, background=3))
    assert (no_global.background, no_global.global_entries, no_global.frames[0].table_row, no_global.frames[0].fill) == (0, 0, 0, 0)
    desc = V.gif_descriptors(p.frames[:3], {2: 0})
    assert desc.dtype == np.int32 and desc.shape == (3, ops.GIF_FRAME_INTS)
    assert desc[1].tolist() == [4, 0, 3, 3, 2, 3, 2, 0, 1, 4, -1] and desc[2].tolist() == [0, 0, 2, 2, -1, 3, 9, 0, 0, 16, 0]
    first3 = V.parse_gif(R.build(4, 4, [R.frame(K.noise(4, 4, 4, 1), disposal=3, transparent=1), R.frame(K.noise(4, 4, 4, 1), disposal=3)], K.palette(4)))
    assert V.gif_descriptors(first3.frames, {})[:, 5:7].tolist() == [[2, 1], [3, 0]]
    assert V.gif_descriptors(V.parse_gif(R.build(4, 4, [R.frame(K.noise(4, 4, 4, 1), disposal=3)], K.palette(4))).frames, {})[0, 5] == 1


def test_background_index_beyond_the_table_has_two_rules_in_pillow_and_is_refused():
    data, W, H, frames, table, background = K.built("background_beyond_table")
    want = R.pillow_frames(data)
    assert not want[1][0, 0].any()                                               # frame 0 is disposed as a palette image: index 9 of 4 entries is black
    assert np.array_equal(want[2][1, 1], table[0]) and table[0].any()            # frame 1 goes through _rgb: entry 0
    with pytest.raises(ValueError, match="frame 0 is disposed to the background index 9"):
        V.parse_gif(data)
    with pytest.raises(ValueError, match="frame 1 is disposed to the background index 9"):
        V.parse_gif(R.build(W, H, [R.frame(frames[0]["indices"], delay=1, table=frames[0]["table"])] + frames[1:], table, background=9))
    harmless = [R.frame(f["indices"], f["left"], f["top"], f["table"], disposal=d, transparent=t, delay=1) for f, d, t in zip(frames, (2, 1, 2), (1, None, None))]
    file = R.build(W, H, harmless, table, background=9)                          # a transparent index, another disposal, the last frame
    assert [f.fill for f in V.parse_gif(file).frames] == [1, 0, 0] and np.array_equal(parsed_frames(file), R.pillow_frames(file))
    inside = K.built("background_inside_table")[0]
    assert [f.fill for f in V.parse_gif(inside).frames] == [2, 2, 2]


def test_parse_gif_refusals():
    g = K.palette(4)
    ok = R.frame(K.noise(2, 2, 4, 1))
    good = R.build(4, 4, [ok], g)
    V.parse_gif(good)
    cases = [
        (R.build(4, 4, [ok], None), "no colour table"),
        (R.build(4, 4, [R.frame(K.noise(2, 2, 4, 1), 3, 0)], g), "outside the logical screen"),
        (R.build(4, 4, [R.frame(K.noise(2, 2, 4, 1), code_size=1)], g), "minimum code size of 1"),
        (R.build(4, 4, [R.frame(K.noise(2, 2, 4, 1), code_size=9, data=b"\x00")], g), "minimum code size of 9"),
        (R.build(4, 4, [R.frame(K.noise(2, 2, 4, 1), transparent=4)], g), "transparent index 4"),
        (R.build(4, 4, [R.frame(np.zeros((0, 2), np.uint8), data=b"\x00")], g), "zero-sized"),
        (R.build(0, 4, [ok], g), "zero-sized logical screen"),
        (R.build(4, 4, [], g), "no image"),
        (good[:-3], "past the end of the file"),
        (good[:15], "past the end of the file"),
        (R.build(4, 4, [ok], K.palette(256))[:400], "past the end of the file"),
        (b"GIF88a" + good[6:], "not a GIF file"),
        (good[:25] + b"\x99" + good[25:], "no extension, image descriptor or trailer"),
    ]
    assert good[25] == 0x2C
    for data, words in cases:
        with pytest.raises(ValueError, match=words):
            V.parse_gif(data)
    with pytest.raises(ValueError, match="decode_gif: .*no colour table"):        # the file is refused before any launch
        V.decode_gif(cases[0][0])


def test_fps_rule():
    cs = lambda *d: [Fraction(x, 100) for x in d]
    assert V.gif_fps(cs(*V.gif_delays(30, 12))) == 30 and sorted(set(V.gif_delays(30, 12))) == [3, 4]
    assert V.gif_fps(cs(4, 4, 4)) == 25 and V.gif_fps(cs(7)) == Fraction(100, 7) and V.gif_fps(cs(*V.gif_delays(Fraction(24000, 1001), 7))) == Fraction(700, 29)
    assert V.gif_fps(cs(3, 5, 3)) is None and V.gif_fps(cs(4, 4, 0)) is None and V.gif_fps(cs(0, 0)) is None and V.gif_fps(cs(10, 40)) is None


# ------------------------------------------------------------------------------------------------------------------------------ the entries
def test_decode_gif_has_no_host_decoder(tmp_path):
    data = K.built("dependent")[0]
    with pytest.raises(EmoHipError, match="no host decoder"):
        V.decode_gif(data, device="cpu")
    with pytest.raises(EmoHipError, match="device tensors"):
        ops.gif_lzw_decode(torch.zeros(8, dtype=torch.uint8), torch.tensor([0, 8]), torch.tensor([8], dtype=torch.int32), torch.tensor([0, 4]), 4)
    with pytest.raises(EmoHipError, match="device tensors"):
        ops.gif_compose(torch.zeros(4, dtype=torch.uint8), torch.tensor([0, 4]), torch.zeros(1, ops.GIF_FRAME_INTS, dtype=torch.int32),
                        torch.zeros(1, 256, 3, dtype=torch.uint8), 1, 2, 2)


def test_layout_is_refused_before_any_launch():
    assert ops.gif_layout_check([0, 10, 10, 25], [8, 2, 5], [0, 100, 101, 2 ** 31 - 1], 28) == 2 ** 31 - 1
    for args, words in ((([0, 10], [], [0, 4], 12), "n=0"), (([0, 10, 5], [8, 8], [0, 4, 8], 12), "ascend inside"),
                        (([0, 10], [8], [0, 4], 8), "ascend inside"), (([-4, 10], [8], [0, 4], 12), "ascend inside"),
                        (([0, 10], [9], [0, 4], 12), "code size of 9"), (([0, 10], [1], [0, 4], 12), "code size of 1"),
                        (([0, 10], [8], [4, 8], 12), "ascend from 0"), (([0, 5, 10], [8, 8], [0, 8, 4], 12), "ascend from 0"),
                        (([0, 5, 10], [8, 8], [0, 2 ** 30, 2 ** 31], 12), "31 bits"), (([0, 10], [8], [0, 0], 12), "31 bits")):
        with pytest.raises(EmoHipError, match=words):
            ops.gif_layout_check(*args)
    assert ops.gif_status_words(0) == "ok" and "End of Information" in ops.gif_status_words(3) and "and" in ops.gif_status_words(12)
    assert sorted(ops.GIF_STATUS) == [R.OK, R.BAD_CODE, R.PAST_END, R.SHORT, R.BAD_INDEX, R.BAD_FRAME]
