"""Host tests of what the clip writers of emote_hack_amd.video_io share (no GPU): the stream layout against a plain loop, the table of
output formats as the single source of every "that option belongs to another format" refusal - of the writers and of the pipeline's
save_path= -, and the one check of the frames."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from emote_hack_amd import video_io as V


# ------------------------------------------------------------------------------------------------------------------------------ layout
def layout_by_hand(bits, head=None, tail=0, totals=None):
    """per row: start = the bytes of the rows before it; per unit: 8 * start + head + the bits before it in its row"""
    bits = np.asarray(bits, np.int64)
    head = np.zeros(len(bits), np.int64) if head is None else np.asarray(head, np.int64)
    offsets, starts, nbytes, start = np.zeros_like(bits), [], [], 0
    for r, row in enumerate(bits):
        before = 0
        for u, b in enumerate(row):
            offsets[r, u] = 8 * start + head[r] + before
            before += int(b)
        total = before if totals is None else int(totals[r])
        starts.append(start)
        nbytes.append((int(head[r]) + total + 7) // 8 + tail)
        start += nbytes[-1]
    return offsets, np.array(starts), np.array(nbytes), (start + 3) // 4 * 4


def check_layout(bits, head=None, tail=0, totals=None, dtype=torch.int32):
    offsets, starts, nbytes, out, got_totals = V._stream_layout(torch.tensor(bits, dtype=dtype), head, tail, totals)
    want = layout_by_hand(bits, head, tail, totals)
    assert offsets.dtype == torch.int64 and offsets.is_contiguous() and np.array_equal(offsets.numpy(), want[0])
    assert np.array_equal(starts, want[1]) and np.array_equal(nbytes, want[2])
    assert out.dtype == torch.uint8 and out.dim() == 1 and out.numel() == want[3] and out.numel() % 4 == 0 and not out.any()
    assert np.array_equal(got_totals, np.asarray(bits).sum(axis=1) if totals is None else totals)
    return out.numel()


def test_stream_layout_equals_a_plain_loop():
    assert check_layout([[5]]) == 4                                              # one row of one unit
    rng = np.random.default_rng(11)
    bits = rng.integers(1, 40, (3, 7))
    bits[0, [0, 3]] = 0                                                          # units of no bits, the first of a row among them
    bits[1, 6] = 0
    bits[1, 0] += 8 - bits[1].sum() % 8                                          # a row that ends on a byte: the next starts right behind it
    assert bits[1].sum() % 8 == 0
    check_layout(bits.tolist())
    check_layout(bits.tolist(), dtype=torch.int64)
    check_layout([[3, 4], [0, 0], [9, 1]])                                       # a row of no bits takes no byte
    check_layout([[0, 0, 0]])
    check_layout(bits.tolist(), head=[0, 1, 17], tail=4)                         # the PNG writer: headers in front, Adler-32 behind
    # the PNG writer knows the totals on the host, and they count bits it adds behind the last unit itself
    check_layout(bits.tolist(), head=[0, 1, 17], tail=4, totals=(bits.sum(axis=1) + [7, 0, 12]).tolist())


def test_stream_layout_of_restart_intervals():
    """n = 2 frames of 5 MCUs at an interval of 2: three intervals per frame, the last one MCU short and padded with blocks of no bits
    (what encode_streams does); a row is an interval, and a frame's first interval starts where the frame before ended"""
    n, n_mcu, ri = 2, 5, 2
    k = -(-n_mcu // ri)
    counts = torch.from_numpy(np.random.default_rng(5).integers(2, 60, (n, n_mcu * 6)).astype(np.int32))
    per = torch.nn.functional.pad(counts.to(torch.int64), (0, (k * ri - n_mcu) * 6)).view(n * k, ri * 6)
    assert per.shape == (6, 12) and not per[2, 6:].any() and not per[5, 6:].any()
    check_layout(per.tolist(), dtype=torch.int64)
    offsets, starts, nbytes, _, totals = V._stream_layout(per)
    blocks = offsets.view(n, k * ri * 6)[:, :n_mcu * 6]                          # the offsets the emit kernel gets: one per real block
    flat = counts.numpy().astype(np.int64)
    for f in range(n):
        for i in range(k):
            first = i * ri * 6
            assert blocks[f, first] == 8 * starts[f * k + i]                     # every interval on a byte
            assert totals[f * k + i] == flat[f, first:first + ri * 6].sum()
            assert np.array_equal(np.diff(blocks[f, first:first + ri * 6].numpy()), flat[f, first:first + ri * 6][:-1])


@pytest.mark.parametrize("total_bytes, length", [(1, 4), (4, 4), (5, 8)])
def test_stream_buffer_is_rounded_up_to_a_dword(total_bytes, length):
    assert check_layout([[8 * total_bytes - 3]]) == length
    assert check_layout([[8] for _ in range(total_bytes)]) == length             # the same bytes as rows of one byte


# ------------------------------------------------------------------------------------------------------------------------------ table
FRAMES = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)                              # on the host: a launch would raise EmoHipError, no ValueError
VALUES = {"quality": 50, "restart_interval": "row"}                              # any other option: 1 (nothing looks at a foreign option's value)
ALL_OPTIONS = sorted({o for r in V.FORMATS.values() for o in r.options})


def owner_of(option):
    return next(r for r in V.FORMATS.values() if option in r.options)


def refusal(call):
    with pytest.raises(ValueError) as e:
        call()
    return str(e.value)


def test_the_table_holds_what_the_writers_knew():
    f = V.FORMATS
    assert [(r.ext, r.format, r.plays, r.sound) for r in f.values()] == [(".avi", None, True, True), (".gif", "gif", True, False),
                                                                        (".apng", "apng", True, False), (".png", "png", False, False)]
    assert f["avi"].options == ("quality", "restart_interval") and f["gif"].options == V.GIF_OPTIONS == ("loop", "colors", "palette", "dither",
                                                                                                         "dither_strength", "strip_rows")
    assert f["apng"].options == V.PNG_OPTIONS == ("filter", "strip_rows", "loop") and f["png"].options == ("filter", "strip_rows")
    assert f["avi"].rate is None and f["gif"].rate is V.gif_delays and f["png"].rate is None
    assert [r.encode for r in f.values()] == [V.encode_avi, V.encode_gif, V.encode_apng, V.encode_png]
    assert set(V.SAVE_KEYWORDS) <= set(ALL_OPTIONS) and all(k.startswith("save_") for k in V.SAVE_KEYWORDS.values())
    with pytest.raises(ValueError, match="65535"):
        f["apng"].rate(65536, 3)


@pytest.mark.parametrize("name", ["avi", "gif", "apng"])
def test_writers_refuse_every_foreign_option_by_its_owner(name, tmp_path):
    record = V.FORMATS[name]
    path = str(tmp_path / f"clip{record.ext}")
    videos, stills = torch.rand(1, 3, 2, 8, 8), [np.zeros((8, 8, 3), np.uint8)]
    foreign = [o for o in ALL_OPTIONS if o not in record.options]
    assert foreign
    for option in foreign:
        kw, owner = {option: VALUES.get(option, 1), "format": record.format}, owner_of(option)
        said = refusal(lambda: V.write_video(FRAMES, path, 25, **kw))
        assert said.startswith("write_video") and f"unknown option {option}= for {record.noun}" in said
        assert f"belong to {owner.noun}" in said and (owner.format is None or f"format=\"{owner.format}\"" in said)
        assert said.replace("write_video", "X") == refusal(lambda: V.save_videos_grid(videos, path, **kw)).replace("save_videos_grid", "X")
        assert said.replace("write_video", "X") == refusal(lambda: V.images2video(stills, path, **kw)).replace("images2video", "X")
    said = refusal(lambda: V.write_video(FRAMES, path, 25, format=record.format, colours=16))      # nobody's option: no owner to name
    assert "unknown option colours=" in said and "belong" not in said
    if not record.sound:
        assert "no sound" in refusal(lambda: V.write_video(FRAMES, path, 25, format=record.format, audio=(np.zeros(10, np.float32), 16000)))
    assert list(tmp_path.iterdir()) == []


def test_write_gif_and_write_apng_are_entries_of_the_same_path(tmp_path):
    for write, record in ((V.write_gif, V.FORMATS["gif"]), (V.write_apng, V.FORMATS["apng"])):
        path = str(tmp_path / f"clip{record.ext}")
        said = refusal(lambda: write(FRAMES, path, 25, quality=50))
        assert "unknown option quality=" in said and f"belong to {V.FORMATS['avi'].noun}" in said
        assert said.split(":", 1)[1] == refusal(lambda: V.write_video(FRAMES, path, 25, format=record.format, quality=50)).split(":", 1)[1]
        assert record.ext in refusal(lambda: write(FRAMES, tmp_path / "clip.avi", 25))
    assert list(tmp_path.iterdir()) == []


def pipeline_without_a_vae():
    from emote_hack_amd import DDIMScheduler
    from emote_hack_amd.pipeline import EMOAnimationPipeline
    return EMOAnimationPipeline(unet=SimpleNamespace(device=torch.device("cpu")), scheduler=DDIMScheduler())


@pytest.mark.parametrize("name", sorted(V.FORMATS))
def test_call_refuses_every_foreign_save_keyword_by_its_owner(name, tmp_path):
    p, record = pipeline_without_a_vae(), V.FORMATS[name]
    path = str(tmp_path / ("f_%04d.png" if name == "png" else f"clip{record.ext}"))
    for option, keyword in V.SAVE_KEYWORDS.items():
        call = lambda: p("", 2, save_path=path, fps=8, **{keyword: VALUES.get(option, 1)})
        if option in record.options:                                             # its own: the checks go on, to the value or to the VAE
            assert f"unknown option {keyword}=" not in refusal(call)
            continue
        said, owner = refusal(call), owner_of(option)
        assert said.startswith("save_path=") and f"unknown option {keyword}= for {record.noun}" in said
        assert f"belong to {owner.noun} (`{owner.ext}` save_path)" in said
    assert list(tmp_path.iterdir()) == []


def test_call_refuses_save_png_filter_with_an_avi_or_a_gif_path(tmp_path):
    """it was ignored there, alone among the save_* keywords"""
    p = pipeline_without_a_vae()
    for name in ("clip.avi", "clip.gif"):
        for value in ("paeth", "adaptive", "best"):
            with pytest.raises(ValueError, match=r"save_png_filter=.*belong to an animated PNG \(`\.apng` save_path\)"):
                p("", 2, save_path=str(tmp_path / name), fps=8, save_png_filter=value)
    with pytest.raises(ValueError, match="VAE"):
        p("", 2, save_path=str(tmp_path / "clip.apng"), fps=8, save_png_filter="paeth")
    assert list(tmp_path.iterdir()) == []


def test_save_plan_knows_path_rate_audio_and_options(tmp_path):
    from fractions import Fraction
    none = dict.fromkeys(V.SAVE_KEYWORDS)
    plan = V.save_plan(tmp_path / "clip.avi", 5, Fraction(25, 2), 2, dict(none, quality=90, restart_interval="row"))
    assert (plan.record, plan.path, plan.rate, plan.options) == (V.FORMATS["avi"], str(tmp_path / "clip.avi"), 25, {"restart_interval": "row"})
    assert plan.record.sound
    plan = V.save_plan(str(tmp_path / "clip.GIF"), 5, Fraction(8), 1, dict(none, loop=3, dither="bayer"))
    assert plan.record is V.FORMATS["gif"] and plan.rate == 8 and plan.options == {"loop": 3, "dither": "bayer"} and not plan.record.sound
    plan = V.save_plan(str(tmp_path / "f_%03d.png"), 5, None, 1, dict(none, filter="up"))
    assert plan.record is V.FORMATS["png"] and plan.rate is None and plan.options == {"filter": "up"}
    assert V.save_plan(str(tmp_path / "clip.apng"), 5, None, 1, none).rate is None       # left to the caller, who asks for fps=
    with pytest.raises(ValueError, match="50 frames per second"):
        V.save_plan(str(tmp_path / "clip.gif"), 5, Fraction(30), 2, none)
    with pytest.raises(ValueError, match="one field"):
        V.save_plan(str(tmp_path / "f_%s.png"), 1, None, 1, none)
    assert list(tmp_path.iterdir()) == []


# ------------------------------------------------------------------------------------------------------------------------------ frames
@pytest.mark.parametrize("encode, what, channels", [(lambda f: V.encode_mjpeg(f), "uint8 RGB frames", 3), (lambda f: V.encode_gif(f, 25), "uint8 RGB frames", 3),
                                                    (lambda f: V.encode_png(f), "uint8 frames", 3), (lambda f: V.encode_apng(f, 25), "uint8 frames", 4)])
def test_one_check_of_the_frames(encode, what, channels):
    good = torch.zeros(2, 8, 8, channels, dtype=torch.uint8)
    too_few_dims = torch.zeros(8, 8, dtype=torch.uint8) if what == "uint8 frames" else good[0]      # the PNG writers take one (H, W, C) frame
    for bad in (good.float(), too_few_dims, torch.zeros(1, 1, 2, 8, 8, channels, dtype=torch.uint8), torch.zeros(2, 8, 8, 2, dtype=torch.uint8),
                good.numpy()):
        with pytest.raises(ValueError, match=what):
            encode(bad)
    with pytest.raises(ValueError, match="no frames"):
        encode(good[:0])
    with pytest.raises(ValueError, match="no frames"):
        encode(good[:0][None])


def test_the_callers_keep_their_own_limits():
    with pytest.raises(ValueError, match="channels"):
        V.encode_png(torch.zeros(1, 8, 8, 2, dtype=torch.uint8))
    with pytest.raises(ValueError, match="65535"):
        V.encode_gif(torch.zeros(1, 65536, 1, 3, dtype=torch.uint8), 25)
    with pytest.raises(ValueError, match="65535"):
        V.quantize_frames(torch.zeros(1, 1, 65536, 3, dtype=torch.uint8))
    for empty in (torch.zeros(1, 0, 4, 3, dtype=torch.uint8), torch.zeros(2, 4, 0, 1, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="at least 1 pixel"):
            V.encode_png(empty)
        with pytest.raises(ValueError, match="1 .. 65535 pixels"):
            V.encode_gif(empty[..., :1].expand(-1, -1, -1, 3), 25)
    frames = V._frames_u8(torch.zeros(1, 3, 4, 5, 3, dtype=torch.uint8), "w")
    assert tuple(frames.shape) == (3, 4, 5, 3)                                   # (1, n, H, W, C) is folded
    assert tuple(V._frames_u8(torch.zeros(4, 5, 1, dtype=torch.uint8), "w", (1, 3, 4), (3, 4, 5)).shape) == (1, 4, 5, 1)
