"""GPU: the device JPEG decoder (univs_amd/jpeg_ops.py, csrc/jpeg_decode.hip) against Pillow's bytes on the corpus of tests/jpeg_cases.py, at
32, 64 and 1024 bits per subsequence; the mixed batch; the chunk-crossing file; the statuses of the malformed files and the fallback's
behaviour on them; the coefficient blocks against `decode_rule` (so that a pixel-stage error is told from an entropy-stage one); the range
conditions on a hand-built file; the readers on files that are not covered."""
import numpy as np
import pytest
import torch

from tests import jpeg_cases as cases
from univs_amd import jpeg_ops
from univs_amd.data import images, jpeg_rule as rule

pytestmark = pytest.mark.gpu
SUBSEQ = (32, 64, 1024)


@pytest.fixture(scope="module")
def corpus():
    """[(case, parsed, Pillow's pixels)], computed once and left unchanged."""
    return [(c, rule.parse_jpeg(c.data), cases.pillow_pixels(c.data)) for c in cases.covered_cases()]


def _groups(corpus):
    groups = {}
    for item in corpus:
        groups.setdefault(jpeg_ops.geometry_key(item[1]), []).append(item)
    return groups


@pytest.mark.parametrize("subseq_bits", SUBSEQ)
def test_every_covered_file_is_pillows_bytes(cuda, corpus, subseq_bits):
    groups = _groups(corpus)
    assert len(groups) >= 20 and sum(len(g) for g in groups.values()) == len(corpus)
    for key, items in groups.items():
        res = jpeg_ops.decode_covered([p for _, p, _ in items], cuda, subseq_bits)
        W, H = key[:2]
        assert res.out.shape == (len(items), H, W, 3) and res.out.dtype == torch.uint8 and res.out.device == cuda
        got = res.out.cpu().numpy()
        for i, (c, p, ref) in enumerate(items):
            assert res.status[i] == 0, (c.name, subseq_bits, jpeg_ops.status_text(int(res.status[i])))
            assert np.array_equal(got[i], ref), (c.name, subseq_bits, int((got[i] != ref).sum()))
        assert res.scratch_bytes > 0 and res.upload_bytes >= sum(len(p.data) - p.ecs[0] for _, p, _ in items)


def test_the_mixed_batch_of_one_size(cuda, corpus):
    batch = cases.same_size_batch()
    assert len(batch) >= 4 and len({rule.parse_jpeg(c.data).restart_interval for c in batch}) == 3      # none, every 3 blocks, every row
    out, status = jpeg_ops.decode_jpegs([c.data for c in batch], cuda)
    assert status.tolist() == [0] * len(batch) and out.shape == (len(batch), 75, 131, 3)
    for i, c in enumerate(batch):
        assert np.array_equal(out[i].cpu().numpy(), cases.pillow_pixels(c.data)), c.name
    # a file of another size in the list is not given to the device; nothing covered is None
    other = next(c for c in cases.covered_cases() if "40x48_420" in c.name)
    out, status = jpeg_ops.decode_jpegs([batch[0].data, other.data, rule.parse_jpeg(batch[1].data)], cuda)
    assert status.tolist() == [0, jpeg_ops.NOT_GIVEN, 0] and np.array_equal(out[2].cpu().numpy(), cases.pillow_pixels(batch[1].data))
    assert jpeg_ops.decode_jpegs(list(cases.uncovered_files().values()), cuda) is None


@pytest.mark.parametrize("subseq_bits", (32, 64))
def test_the_chunk_crossing_file(cuda, subseq_bits):
    c = cases.chunk_crossing()
    p = rule.parse_jpeg(c.data)
    (one,), _ = rule.unstuff(p.data, p.ecs[0])
    assert 8 * len(one) > 1024 * subseq_bits                        # more subsequences than the workgroup has lanes
    res = jpeg_ops.decode_covered([p], cuda, subseq_bits)
    assert res.status.tolist() == [0] and 1 <= res.rounds[0] <= 1023
    assert np.array_equal(res.out[0].cpu().numpy(), cases.pillow_pixels(c.data))
    assert np.array_equal(res.blocks[0].cpu().numpy(), rule.decode_blocks(p))


def test_the_block_buffer_is_the_rules(cuda, corpus):
    picked = [next(x for x in corpus if x[0].name.startswith("restart3_75x131_420")), next(x for x in corpus if x[0].name.startswith("noise_17x31_422")
                                                                                          or x[0].name.startswith("smooth_17x31_422"))]
    for c, p, _ in picked:
        for sb in (32, 1024):
            res = jpeg_ops.decode_covered([p], cuda, sb)
            assert np.array_equal(res.blocks[0].cpu().numpy(), rule.decode_blocks(p)), (c.name, sb)


def test_malformed_files_have_their_statuses_and_fall_back_to_the_host_reader(cuda):
    bad = cases.malformed_files()
    expect = {"truncated at the first entropy byte": 512, "truncated in the middle": 512, "truncated before EOI": 512, "truncated in the last bytes": 512,
              "more blocks than data": 16, "dri doubled": 32, "dri removed": 32}
    for name, data in bad.items():
        p = rule.parse_jpeg(data)
        host_kind, host_value = cases.host_read(data)
        if not rule.covered(p):
            assert name in ("truncated in the headers", "huffman count overflow") and jpeg_ops.decode_jpegs([data], cuda) is None
        else:
            for sb in (32, 1024):
                out, status = jpeg_ops.decode_jpegs([p], cuda, sb)
                if name in expect:
                    assert status[0] > 0 and status[0] & expect[name], (name, sb, int(status[0]))
                if status[0] == 0:                                   # status OK: then the pixels are Pillow's
                    assert host_kind == "pixels" and np.array_equal(out[0].cpu().numpy(), host_value), (name, sb)
            assert name != "flipped bit" or status[0] == 0
        # through the reader: the host reader's own behaviour, exception or pixels
        told = []
        reader = lambda k, data=data: cases.pillow_pixels(data)      # noqa: E731
        if host_kind == "raises":
            with pytest.raises(host_value):
                jpeg_ops.decode_runs([data], cuda, reader, on_fallback=lambda k, why: told.append(why))
            assert len(told) == 1
        else:
            runs = jpeg_ops.decode_runs([data], cuda, reader, on_fallback=lambda k, why: told.append(why))
            assert len(runs) == 1 and np.array_equal(runs[0][0].cpu().numpy(), host_value), name


def test_the_range_conditions_set_the_not_covered_status(cuda):
    data = cases.oversized_product()
    p = rule.parse_jpeg(data)
    assert rule.covered(p) and not rule.decode_rule(p).in_range
    res = jpeg_ops.decode_covered([p], cuda)
    assert res.status.tolist() == [256]
    assert np.array_equal(res.blocks[0].cpu().numpy(), rule.decode_blocks(p))       # the entropy stage is fine; the product leaves int16
    told = []
    runs = jpeg_ops.decode_runs([data], cuda, lambda k: cases.pillow_pixels(data), on_fallback=lambda k, why: told.append(why))
    assert len(told) == 1 and "256" in told[0] and np.array_equal(runs[0][0].cpu().numpy(), cases.pillow_pixels(data))


def test_read_images_decodes_covered_files_and_falls_back_for_the_rest(cuda, tmp_path):
    files = [cases.same_size_batch()[0].data, cases.same_size_batch()[1].data] + list(cases.uncovered_files().values()) + \
            [next(c for c in cases.covered_cases() if "16x16_grey" in c.name).data]
    paths = []
    for i, data in enumerate(files):
        paths.append(str(tmp_path / f"{i:02d}.jpg"))
        open(paths[-1], "wb").write(data)
    for fmt in ("RGB", "BGR"):
        got = images.read_images(paths, decode="gpu", device=cuda, format=fmt)
        assert len(got) == len(paths)
        for t, path in zip(got, paths):
            ref = images.read_image(path, fmt)                       # (the EXIF-rotated file comes out rotated)
            assert t.device == cuda and t.dtype == torch.uint8 and np.array_equal(t.cpu().numpy(), ref), path
    runs = images.decoded_runs(paths, cuda)
    assert [len(r) for r in runs] == [2, 1, 1, 1, 1, 1]              # the two frames of one size are one run, a view of one launch's output
