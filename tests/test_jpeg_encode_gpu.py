"""GPU: the device JPEG encoder (univs_amd/jpegenc_ops.py, csrc/jpeg_encode.hip) against the encoder rule, and therefore Pillow
(tests/test_jpeg_encode_rule_cpu.py holds the rule to Pillow's bytes on the same corpus): every case of tests/jpeg_encode_cases.py, the
coefficient blocks (so that a transform error is told from an entropy-coding one), a batch against its single calls, a frame that takes
several pack workgroups and several steps of the stuffing, the smallest frames, and the round trip through the device decoder."""
import numpy as np
import pytest
import torch

from tests import jpeg_cases, jpeg_encode_cases as cases
from univs_amd import jpeg_ops, jpegenc_ops
from univs_amd.data import jpeg_encode_rule as rule

pytestmark = pytest.mark.gpu

# csrc/jpeg_encode.hip: JPEGENC_PACK_BLOCKS, JPEGENC_STUFF_STEP, the blocks of a jpegenc_blocks_kernel workgroup, JPEGENC_SCAN_THREADS
PACK_BLOCKS, STUFF_STEP, BLOCKS_PER_WG, SCAN_THREADS = 128, 4096, 32, 1024


@pytest.fixture(scope="module")
def expected():
    """{case name: the rule's file}, computed once and left unchanged."""
    return {c.name: rule.encode_rule(c.rgb, c.quality, c.sampling) for c in cases.corpus()}


def _groups():
    groups = {}
    for c in cases.corpus():
        groups.setdefault((c.rgb.shape[:2], c.quality, c.sampling), []).append(c)
    return groups


def test_every_case_of_the_corpus_is_the_rules_file(cuda, expected):
    groups = _groups()
    assert sum(len(g) for g in groups.values()) == len(cases.corpus()) >= 540
    for (size, quality, sampling), items in groups.items():           # the contents of one size, quality and sampling: one call
        rgb = torch.from_numpy(np.stack([c.rgb for c in items])).to(cuda)
        files = jpegenc_ops.encode_jpegs(rgb, quality, sampling)
        for c, data in zip(items, files):
            assert isinstance(data, bytes) and data == expected[c.name], (c.name, len(data), len(expected[c.name]))


@pytest.mark.parametrize("sampling", cases.SAMPLINGS)
def test_the_coefficient_blocks_are_the_rules(cuda, sampling):
    for name in (f"noise_75x131_{sampling}_q90", f"patches_17x31_{sampling}_q100", f"smooth_7x9_{sampling}_q5"):
        c = next(c for c in cases.corpus() if c.name == name)
        res = jpegenc_ops.encode_covered(torch.from_numpy(c.rgb.copy())[None].to(cuda), c.quality, c.sampling)
        ref = rule.scan_blocks(c.rgb, c.quality, c.sampling)
        assert res.status.tolist() == [0]
        got = res.blocks[0].cpu().numpy()
        assert got.shape == ref.coef.shape and np.array_equal(got, ref.coef), (name, np.flatnonzero((got != ref.coef).any(1))[:8])
        coded = rule.entropy_code(ref)
        assert (int(res.totals[0]) + 7) // 8 == len(coded.data) - coded.stuffed and res.data[0] == coded.data


def test_a_batch_of_three_frames_is_the_three_single_calls(cuda):
    frames = np.stack([jpeg_cases.content(kind, 75, 131, 3800 + i) for i, kind in enumerate(jpeg_cases.CONTENTS)])
    rgb = torch.from_numpy(frames).to(cuda)
    batch = jpegenc_ops.encode_jpegs(rgb, 90, "420")
    singles = [jpegenc_ops.encode_jpegs(rgb[i:i + 1], 90, "420")[0] for i in range(3)]
    assert batch == singles and len(set(batch)) == 3
    assert batch == [cases.pillow_file(f, 90, "420") for f in frames]


@pytest.mark.parametrize("sampling", cases.SAMPLINGS)
def test_a_frame_of_several_pack_workgroups_and_stuffing_steps(cuda, sampling):
    a = jpeg_cases.content("noise", 200, 264, 3900)
    ref = rule.scan_blocks(a, 90, sampling)
    coded = rule.entropy_code(ref)
    # 25 x 33 luma blocks and the chroma: more blocks than one pack workgroup and one step of the scan own, more bytes than one step of
    # the stuffing workgroup moves, and FF bytes to stuff in more than one step
    assert len(ref.coef) > 2 * PACK_BLOCKS and len(ref.coef) > SCAN_THREADS and len(ref.coef) > BLOCKS_PER_WG
    assert len(coded.data) - coded.stuffed > 2 * STUFF_STEP and coded.stuffed > 2
    res = jpegenc_ops.encode_covered(torch.from_numpy(a)[None].to(cuda), 90, sampling)
    assert res.status.tolist() == [0] and res.data[0] == coded.data
    assert res.stream_bytes == len(coded.data) and res.scratch_bytes < 208 * len(ref.coef) * 2       # sized from the totals, not the worst case
    assert jpegenc_ops.encode_jpegs(torch.from_numpy(a)[None].to(cuda), 90, sampling) == [cases.pillow_file(a, 90, sampling)]


@pytest.mark.parametrize("size", ((1, 1), (7, 9)))
def test_the_smallest_frames(cuda, size):
    for sampling in cases.SAMPLINGS:
        for quality in (1, 50, 100):
            a = jpeg_cases.content("noise", size[0], size[1], 4000 + quality)
            assert jpegenc_ops.encode_jpegs(torch.from_numpy(a)[None].to(cuda), quality, sampling) == [cases.pillow_file(a, quality, sampling)]


def test_no_frames_and_what_the_entry_does_not_cover(cuda):
    assert jpegenc_ops.encode_jpegs(torch.empty((0, 8, 8, 3), dtype=torch.uint8, device=cuda)) == []
    a = jpeg_cases.content("smooth", 16, 16, 4100)
    # quality 0 is outside the entry's coverage: Pillow encodes it
    assert jpegenc_ops.encode_covered(torch.from_numpy(a)[None].to(cuda), 0, "420") is None
    assert jpegenc_ops.encode_jpegs(torch.from_numpy(a)[None].to(cuda), 0, "420") == [cases.pillow_file(a, 0, "420")]
    with pytest.raises(ValueError, match="sampling"):
        jpegenc_ops.encode_jpegs(torch.from_numpy(a)[None].to(cuda), 90, "411")


def test_the_device_decoder_reads_what_the_device_encoder_wrote(cuda):
    from PIL import Image
    import io
    for sampling in cases.SAMPLINGS:
        frames = np.stack([jpeg_cases.content(kind, 40, 48, 4200 + i) for i, kind in enumerate(jpeg_cases.CONTENTS)])
        files = jpegenc_ops.encode_jpegs(torch.from_numpy(frames).to(cuda), 90, sampling)
        out, status = jpeg_ops.decode_jpegs(files, cuda)
        assert status.tolist() == [0, 0, 0]
        for i, data in enumerate(files):
            with Image.open(io.BytesIO(data)) as im:
                assert np.array_equal(out[i].cpu().numpy(), np.asarray(im.convert("RGB"))), (sampling, i)
