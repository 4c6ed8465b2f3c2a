"""CPU: the wave rectangles that the read-back of the per-wave mask table
reports (rt_debug_wave_rects, the host side of rt_debug_wave_masks; DESIGN.md
§3.29).  For every lanes-per-pixel form, whole frames and interleaved rows,
frames whose sides are and are not multiples of the workgroup tile: every pixel
of the partition's rows lies in exactly one rectangle, every rectangle has the
form's shape, and the order is wave row-major."""
import numpy as np
import pytest

from gpuraytracer_amd.host import wave_rects

# (lanes, rows interleaved) -> pixels per wave (wide, high)
SHAPES = {(1, False): (8, 8), (4, False): (4, 4), (16, False): (2, 2),
          (1, True): (8, 8), (4, True): (16, 1), (16, True): (4, 1)}
FRAMES = [(96, 72), (70, 45), (1, 1), (33, 7)]
ROWS = [(0, 1, 0), (1, 3, 0), (2, 5, 3), (0, 2, 0)]  # row_start, row_step, row_count (0: every row)


def partition_rows(h, start, step, count):
    rows = list(range(start, h, step))
    return rows[:count] if count else rows


CASES = [(w, h, start, step, count) for w, h in FRAMES for start, step, count in ROWS
         if start < h and (not count or start + (count - 1) * step < h)]  # partitions inside the frame
assert len(CASES) == 13 and {c[:2] for c in CASES} == set(FRAMES)


@pytest.mark.parametrize("lanes", [1, 4, 16])
@pytest.mark.parametrize("w,h,start,step,count", CASES)
def test_every_pixel_in_exactly_one_rectangle(lanes, w, h, start, step, count):
    rows = partition_rows(h, start, step, count)
    r = wave_rects(w, h, lanes, start, step, count)
    ww, wh = SHAPES[(lanes, step > 1)]
    assert r.shape[1] % 2 == 0 and r.shape[0] % 2 == 0, "whole workgroups of 2 x 2 waves"
    assert r.shape[1] * ww >= w and (r.shape[1] - 2) * ww < w
    assert r.shape[0] * wh >= len(rows) and (r.shape[0] - 2) * wh < len(rows)
    assert not r["cam_mask"].any() and not r["shd_mask"].any()
    covered = np.zeros((h, w), np.int32)
    for wy in range(r.shape[0]):
        for wx in range(r.shape[1]):
            q = r[wy, wx]
            assert (q["x0"], q["x1"]) == (wx * ww, wx * ww + ww - 1)
            assert q["y0"] == start + wy * wh * step and q["y1"] == q["y0"] + (wh - 1) * step
            ys = [y for y in range(q["y0"], q["y1"] + 1, step) if y < h and y in rows]
            for y in ys:
                covered[y, q["x0"]:min(q["x1"], w - 1) + 1] += 1
    want = np.zeros((h, w), np.int32)
    want[rows] = 1
    assert np.array_equal(covered, want)


def test_bad_arguments():
    from gpuraytracer_amd import RtError
    for args in ((0, 4, 4), (4, 4, 3), (4, 4, 4, 4), (4, 4, 4, 0, 1, 5)):
        with pytest.raises(RtError):
            wave_rects(*args)
