"""GPU: the Halton low-digit tables made once per context (rt_create_ex) and
copied into LDS by the box-cluster kernel's workgroups.  The
context's device buffer is read back and compared bit for bit with the host
table (tests/test_halton_table_once.py holds that one against the reference
loop); Cornell 64x48 is rendered with the tables on and off against the
oracle; two contexts made one after the other own a buffer each and render
the same frame."""
import ctypes

import numpy as np
import pytest

import oracle_lib
from gpuraytracer_amd import Options, RenderParams, Renderer, Scene, seed_splitmix
from gpuraytracer_amd._native import lib
from test_gpu_camera_candidates import CLUSTER_KERNEL, same_bits
from test_halton_table_once import TOTAL, host_table

pytestmark = pytest.mark.gpu
W, H = 64, 48


def device_table(r):
    tab = np.full(TOTAL, np.nan, np.float32)
    assert lib.rt_debug_halton_table_device(r._ctx, tab.ctypes.data_as(ctypes.c_void_p), tab.size) == 0
    return tab


@pytest.fixture(scope="module")
def cornell():
    return Scene.cornell_box(W, H), seed_splitmix(W, H, key=19)


def test_device_buffer_equals_host_table(cornell):
    s, sd = cornell
    host = host_table()[0]
    with Renderer(s, seeds=sd) as r:
        dev = device_table(r)
        short = np.zeros(TOTAL - 1, np.float32)
        assert lib.rt_debug_halton_table_device(r._ctx, short.ctypes.data_as(ctypes.c_void_p), short.size) != 0
    assert np.array_equal(dev.view(np.uint32), host.view(np.uint32))


@pytest.mark.parametrize("spp,tables", [(32, 1), (4, 0)])
def test_cornell_tables_on_and_off(cornell, spp, tables):
    """4 lanes per pixel: 32 spp are 8 rounds per lane (tables on), 4 spp one (off)."""
    s, sd = cornell
    with Renderer(s, seeds=sd, options=Options(lanes=4)) as r:
        out = r.render(RenderParams(spp=spp, bounces=3))
        info = r.last_launch()
    assert CLUSTER_KERNEL % 3 in info["kernel"] and info["lanes_per_pixel"] == 4, info
    assert info["halton_tables"] == tables, info
    same_bits(out, oracle_lib.render(s, sd, spp, 3), f"{spp} spp")


def test_two_contexts_own_their_tables(cornell):
    s, sd = cornell
    frames, tabs = [], []
    for _ in range(2):
        with Renderer(s, seeds=sd, options=Options(lanes=4)) as r:
            tabs.append(device_table(r))
            frames.append(r.render(RenderParams(spp=32, bounces=3)))
            assert r.last_launch()["halton_tables"] == 1
    with Renderer(s, seeds=sd, options=Options(lanes=4)) as a, Renderer(s, seeds=sd, options=Options(lanes=4)) as b:
        both = [b.render(RenderParams(spp=32, bounces=3)), a.render(RenderParams(spp=32, bounces=3))]
        tabs += [device_table(a), device_table(b)]
    for f in frames[1:] + both:
        same_bits(f, frames[0], "frames of two contexts")
    for t in tabs[1:]:
        assert np.array_equal(t.view(np.uint32), tabs[0].view(np.uint32))
