#!/usr/bin/env python3
"""Hash of the RENDER path's device-side sources: ties profiles/traffic_*.json - PMC counters of the render kernels - to the build they
were measured on.  Everything under fidget_amd/csrc counts (generators of the assembly kernels, HIP kernels, the fragments of the C ABI
with the frame driver, headers) except the files only the mesh path uses (MESH_ONLY).  Those are reached from capi.hip through two files
alone: capi_mesh.hpp - the mesher's part of the C ABI, with capi_mesh_util.hpp (what the mesh path's fragments share) at its top and
the list of the other fragments, one capi_X.hpp per subject, at its end - and mesh.hip with the headers and kernel files it includes
(tests/test_mesh_fragments.py).  A change there cannot alter a render kernel or how a frame is launched."""
import glob, hashlib, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH_ONLY = ("mesh.hip", "mesh_collapse.hpp", "mesh_qef.hpp", "mesh_edges.hpp", "mesh_walk.hpp", "host_mesh.hpp", "capi_mesh.hpp", "capi_mesh_util.hpp", "capi_voxels.hpp", "capi_contour.hpp", "capi_cc.hpp", "mesh_split.hpp", "mesh_vox.hpp", "mesh_cc.hpp", "mesh_edt.hpp", "edt.hip", "capi_edt.hpp", "mesh_thick.hpp", "thick.hip", "capi_thick.hpp", "mesh_vmesh.hpp", "vmesh.hip", "capi_vmesh.hpp", "mesh_flow.hpp", "flow.hip", "capi_flow.hpp", "mesh_trivox.hpp", "trivox.hip", "capi_trivox.hpp", "mesh_topo.hpp", "topo.hip", "capi_topo.hpp", "mesh_outline.hpp", "outline.hip", "capi_outline.hpp", "mesh_nest.hpp", "nest.hip", "capi_nest.hpp", "mesh_slice.hpp", "slice.hip", "capi_slice.hpp", "mesh_slice_nest.hpp", "slice_nest.hip", "capi_slice_nest.hpp")


def source_hash(root=ROOT):
    h = hashlib.sha1()
    for f in sorted(glob.glob(os.path.join(root, "fidget_amd", "csrc", "*"))):
        name = os.path.basename(f)
        if os.path.isfile(f) and name.rsplit(".", 1)[-1] in ("py", "hip", "hpp", "h", "cpp") and name not in MESH_ONLY:
            h.update(name.encode())
            h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


if __name__ == "__main__":
    print(source_hash())
