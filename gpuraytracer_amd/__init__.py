"""gpuraytracer_amd — MI355X-native drop-in for the ``pathTrace`` hot path of
Nishad-Sharma/gpuRaytracer.

The product is ``librtpt.so`` (HIP kernel for gfx950 + the C-ABI of
``include/rtpt.h``).  This package is the Python host mirror of the
reference's Swift host API, used by the tests and ``bench.py``:

* :class:`Scene` — ``RTrace/scene.swift`` (``initCornellBox`` and the
  config-4 sphere field), holding the ``shaderTypes.h`` arrays.
* :class:`Renderer` — ``RTrace/renderer.swift`` (``init`` uploads the scene and
  the seed texture, ``draw`` dispatches and waits); ``trace_rays`` answers
  batches of the caller's own rays (closest hit / any hit) through the same
  acceleration structures; ``render_aov`` gives the first-hit feature buffers
  (albedo, normal, depth, coverage, primitive id) of the beauty samples;
  ``denoise`` / ``render_denoised`` filter a low-spp render with them;
  ``render_counts`` renders one sample count per pixel, ``plan_samples`` makes
  such counts from a pilot render and ``render_adaptive`` runs the pipeline;
  ``trace_paths`` path-traces radiance along the caller's own rays;
  ``reproject`` / ``render_temporal`` carry accumulated colour from frame to
  frame under a moving camera.

There is no CPU fallback: importing fails loudly when ``librtpt.so`` has not
been built (``make`` or ``__graft_entry__.build()``), and rendering fails
loudly without a HIP device.
"""
from __future__ import annotations

from ._native import (ABI_VERSION, RT_AOV_CENTER, RT_RAYS_CHUNK, AovBuffers, AovParams, CameraGPU, DenoiseBuffers,
                      DenoiseParams, MaterialGPU, PathParamsC, PlanParams, PlanStats, RT_PLAN_RELATIVE, ReprojectBuffers, ReprojectParams, RtError, SphereGPU, SquareLightGPU, float3, lib, library_path)
from .host import (DEFAULT_SEED_KEY, MisParams, Options, RenderParams, Renderer, Scene, comm_unique_id,
                   math_sums, math_values, place_tiles_host, plan_samples_host, reproject_host, seed_splitmix, tile_layout, tonemap_rgba8)

__all__ = [
    "ABI_VERSION", "CameraGPU", "MaterialGPU", "SphereGPU", "SquareLightGPU", "float3",
    "RtError", "lib", "library_path", "Scene", "Renderer", "RenderParams", "MisParams",
    "DEFAULT_SEED_KEY", "seed_splitmix", "tonemap_rgba8", "comm_unique_id", "tile_layout",
    "place_tiles_host", "RT_RAYS_CHUNK", "RT_AOV_CENTER", "AovParams", "AovBuffers",
    "DenoiseParams", "DenoiseBuffers", "math_values", "math_sums", "PlanParams", "PlanStats",
    "RT_PLAN_RELATIVE", "plan_samples_host", "PathParamsC", "ReprojectParams", "ReprojectBuffers", "reproject_host",
]
