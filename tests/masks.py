"""Edge masks shared by the test files (no imports beyond numpy, so that light modules can use them)."""
import numpy as np


def basin(mesh, K):
    """A bathymetry-like maxLevelEdgeTop.  s = xEdge scaled to [0, 1] on planar meshes, (1 + zEdge / radius) / 2 on the sphere;
    f = 1.3 s - 0.15; maxLevelEdgeTop[e] = clip(rint(K f), 0, K): land (0), full columns (K) and every depth between; on the periodic
    planar mesh a cliff from K to 0."""
    if getattr(mesh, "on_sphere", False):
        s = (1.0 + np.asarray(mesh.zEdge) / mesh.sphere_radius) / 2.0
    else:
        x = np.asarray(mesh.xEdge, dtype=np.float64)
        s = (x - x.min()) / (x.max() - x.min())
    return np.clip(np.rint(K * (1.3 * s - 0.15)), 0, K).astype(np.int32)
