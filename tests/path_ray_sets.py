"""The chosen ray set of the path-query tests (tests/test_paths.py states its
properties on the CPU, tests/test_gpu_paths.py traces it on the GPU) and the
camera rays of a frame as rt_ray rows.

1003 rays, so that blocks of 64 (a wave), 16 (a DPP row's share of a wave at 16
lanes per ray: 4 rays) and 4 all leave a tail.  By index:

  [0, 384)      interior origins, generic directions (ray_sets B)
  [384, 448)    towards the camera: rays that leave through the room's open side
  [448, 512)    aimed at points of the light
  [512, 584)    at the first 36 triangles from 0.05 off either side of each
  [584, 648)    a known hit with tmax at it (the strict bound drops it)
  [648, 712)    a known hit with tmin at it
  [712, 896)    generic rays, every third one replaced by an out-of-domain
                variant of itself: waves that hold traced and untraced rays,
                and 16-lane rows whose neighbours differ
  [896, 960)    64 consecutive out-of-domain rays: at one lane per ray a whole
                wave without a ray in the domain
  [960, 1003)   generic rays again; the last workgroup, wave and row are partial
"""
import numpy as np

import aov_ref
import pt_oracle_np as onp
import ray_sets

f32 = np.float32
N_RAYS = 1003
OUT_MIXED = (712, 896)
OUT_BLOCK = (896, 960)


def camera_rays(sc, seeds, n):
    """The camera rays of sample n of every pixel, row-major, as (H*W, 8) rt_ray
    rows with tmin 0.001 and tmax 1000, and the seeds flattened alike."""
    yy, xx = np.meshgrid(np.arange(sc.H), np.arange(sc.W), indexing="ij")
    xs, ys = xx.ravel(), yy.ravel()
    sd = np.asarray(seeds, np.uint32).reshape(sc.H, sc.W)[ys, xs]
    i = (sd.astype(np.uint64) + np.uint64(n)).astype(np.uint32)
    o, d = aov_ref.camera_rays(sc, xs, ys, onp.halton(i, 0), onp.halton(i, 1))
    return ray_sets.pack(np.stack([o.x, o.y, o.z], -1), np.stack([d.x, d.y, d.z], -1), f32(0.001), f32(1000.0)), sd


def ray_set(scene, sc, dom):
    """(rays (1003, 8) float32, out_of_domain bool[1003]) for a scene."""
    B, _ = ray_sets.sets_bc()
    r = B[:N_RAYS].copy()
    rng = np.random.default_rng(77)
    o = B[1024:1024 + 64, 0:3]
    # through the open side: the camera looks into the room through it
    cam = np.array([sc.pos.x, sc.pos.y, sc.pos.z], f32)
    aim = cam + rng.uniform(-0.5, 0.5, (64, 3)).astype(f32)
    r[384:448] = ray_sets.pack(o, ray_sets._unit(aim - o), f32(0.001), f32(1000.0))
    # at the light, from below it
    lc = np.array([sc.lc.x, sc.lc.y, sc.lc.z], f32)
    q = np.tile(lc, (64, 1))
    q[:, 0] += rng.uniform(-0.2, 0.2, 64).astype(f32)
    q[:, 2] += rng.uniform(-0.2, 0.2, 64).astype(f32)
    ol = B[2048:2048 + 64, 0:3].copy()
    ol[:, 1] = np.minimum(ol[:, 1], lc[1] - f32(0.5))
    r[448:512] = ray_sets.pack(ol, ray_sets._unit(q - ol), f32(0.001), f32(1000.0))
    # at each of the first 36 triangles, from 0.05 off its centroid on either side
    v = ray_sets._tri_vertices(scene)
    v = v[np.arange(36) % len(v)]  # a scene with fewer: again from the first
    c =(v[:, 0] + v[:, 1] + v[:, 2]) / f32(3.0)
    nrm = ray_sets._unit(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]).astype(f32))
    r[512:548] = ray_sets.pack(c + f32(0.05) * nrm, -nrm, f32(0.001), f32(1000.0))
    r[548:584] = ray_sets.pack(c - f32(0.05) * nrm, nrm, f32(0.001), f32(1000.0))
    # a known hit with tmax / tmin exactly at it
    t, ids = ray_sets.reference(sc, B[:384])
    assert np.count_nonzero(ids >= 0) >= 128
    r[584:648] = ray_sets.d_tmax_at_hit(B[:384], t, ids)[:64]
    r[648:712] = ray_sets.d_tmin_at_hit(B[:384], t, ids)[64:128]
    # out-of-domain rays of every kind
    out = np.zeros(N_RAYS, bool)
    out[OUT_MIXED[0]:OUT_MIXED[1]:3] = True
    out[OUT_BLOCK[0]:OUT_BLOCK[1]] = True
    k = np.flatnonzero(out)
    r[k] = ray_sets.out_of_domain_variants(r[k], dom["origin_max"])
    return r, out
