"""Hand-built sphere scenes for the degenerate inputs of the sphere BVH walks
(tests/test_sphere_edge_layout.py on the CPU, tests/test_gpu_sphere_edges.py
on the GPU).

Every scene is the ``Scene.random_spheres`` room with no random sphere -- 12
wall and light triangles, the camera at (0, 0, 9) looking down -z, the light
centre at (0, 2.49, 0) -- plus a fixed list of spheres.  A sphere is diffuse
(0.7, 0.3, 0.2, w = 1), roughness 1, not emissive, unless its row says so.
"""
import math

from gpuraytracer_amd import Scene, SphereGPU

CAMERA = (0.0, 0.0, 9.0)
LIGHT = (0.0, 2.49, 0.0)
ALBEDO = (0.7, 0.3, 0.2)
NAN, INF = math.nan, math.inf

# name -> rows (centre, radius[, emissive]); what each forces on the builder and the walks
ROWS = {
    # a root-leaf tree: n_sphere_nodes == 1
    "single": [((0, 0, 0), 1.0)],
    # the smallest inner node
    "two": [((-1, 0, 0), 0.7), ((1, 0, 0), 0.7)],
    # every camera ray starts inside a sphere: the t2 root, a hit from inside
    "camera_inside": [(CAMERA, 0.5), ((0, 0, 0), 0.8)],
    # every ray origin of the render lies inside a box that contains the scene
    "room_inside": [((0, 0, 0), 100.0), ((0, 0, 0), 0.8)],
    # coincident centroids in the SAH sweep, an exact duplicate, nested boxes
    "concentric": [((0, -1, 0), 0.9), ((0, -1, 0), 0.6), ((0, -1, 0), 0.3), ((0, -1, 0), 0.9)],
    # fabsf(radius) in the builder against r*r in the test; a radius below the
    # culling margin and below the 1e-3 offset of the bounce origin
    "neg_zero_tiny": [((-1, 0, 0), -0.6), ((1, 0, 0), 0.0), ((0, 1, 0), 1e-4), ((0, -1, 0), 0.5)],
    # tangent neighbours, equal coordinates on every sort axis, ties in t
    "lattice": [((0.5 * x, 0.5 * y, 0.5 * z), 0.25)
                for x in range(-3, 4) for y in range(-3, 4) for z in range(-3, 4)],
    # the light-hit overwrite and break for a sphere
    "emissive": [((0, 0, 0), 0.6, (2.0, 1.0, 0.5)), ((1.2, -1, 0), 0.6)],
    # the shadow any-hit is true almost everywhere; a sphere cuts the ceiling
    "cover_light": [(LIGHT, 0.8), ((0, -1, 0), 0.6)],
    # cancellation in the discriminant; fp16 boxes at 2e4
    "huge": [((0, -10002, 0), 10000.0), ((0, 0, 0), 0.5)],
    # a non-finite inner box: both compact tables are refused
    "nonfinite": [((0, 0, 0), NAN), ((1, 0, 0), INF), ((-1, 0, 0), 0.5)],
    # a non-finite root leaf: only the leaf-box table is refused
    "nan_single": [((0, 0, 0), NAN)],
}
NAMES = list(ROWS)


def room(width, height):
    """The room alone (no sphere)."""
    return Scene.random_spheres(width, height, 0)


def with_spheres(base, rows):
    """``base``'s room with the spheres of ``rows``."""
    sph = (SphereGPU * len(rows))()
    for s, row in zip(sph, rows):
        (s.center.x, s.center.y, s.center.z), s.radius = row[0], row[1]
        m = s.material
        m.diffuse.x, m.diffuse.y, m.diffuse.z = ALBEDO
        m.diffuse.w = 1.0
        m.roughness = 1.0
        if len(row) > 2:
            m.emissive.x, m.emissive.y, m.emissive.z = row[2]
    return Scene(base.camera, base.materials, base.vertices, base.light, sph)


def build(name, width, height, rows=None):
    """Scene ``name`` of the table at ``width`` x ``height`` (``rows``: a
    subset of its sphere rows)."""
    return with_spheres(room(width, height), ROWS[name] if rows is None else rows)
