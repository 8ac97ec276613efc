//! `fidget_mesh::Octree::build(..).walk_dual()` as one call (`fhip_mesh_build`): cell classification, leaf sampling, octree
//! assembly (check_done / collapsible, octree.rs:256-470) and the dual walk (dc.rs) all run on the device; the host receives the
//! finished `Mesh`, the single-threaded recursion's, element for element.
use fidget_core::shape::BoundShape;
use fidget_mesh::{Mesh, Settings};

use crate::{axis_slots, ffi, var_key, HipFunction, CTX};

/// Builds the mesh of `shape` at `settings.depth`; `None` when the variables do not bind or the build fails
pub fn mesh(b: BoundShape<HipFunction, f32>, settings: &Settings) -> Option<Mesh> {
    let f = b.shape().inner();
    let tape = f.tape();
    let m = settings.world_to_model.transpose();
    let axes = axis_slots(fidget_core::eval::Function::vars(f));
    let mut keys = vec![];
    let mut vals = vec![];
    for (k, v) in b.vars() {
        keys.push(var_key(*k));
        vals.push(*v);
    }
    let mut h = std::ptr::null_mut();
    let st = CTX.with(|c| unsafe {
        ffi::fhip_mesh_build(c.raw(), tape.raw(), settings.depth as u32, m.as_ptr(), axes.as_ptr(), keys.as_ptr(), vals.as_ptr(),
                             keys.len() as u32, &mut h)
    });
    if st != 0 {
        return None;
    }
    let mut n = [0u64; 8];
    unsafe { ffi::fhip_mesh_counts(h, n.as_mut_ptr()) };
    let mut vertices = vec![nalgebra::Vector3::<f32>::zeros(); n[6] as usize]; // repr(C) [f32; 3]
    let mut triangles = vec![nalgebra::Vector3::<usize>::zeros(); n[7] as usize]; // [u64; 3] on 64-bit targets
    unsafe {
        ffi::fhip_mesh_vertices(h, vertices.as_mut_ptr().cast());
        ffi::fhip_mesh_triangles(h, triangles.as_mut_ptr().cast());
        ffi::fhip_mesh_free(h);
    }
    Some(Mesh { vertices, triangles })
}

/// A mesh that stays with the library after the build, for what a caller does with it on the device: `Mesh::write_stl`
/// (fidget-mesh/src/output.rs:5-38) and gradients at its vertices.  Built with context option `mesh_keep_device`, so both read the arrays
/// where the dual walk left them.
pub struct DeviceMesh {
    h: *mut ffi::fhip_mesh,
}

impl DeviceMesh {
    /// As `mesh`, but the handle is kept; `None` when the variables do not bind or the build fails
    pub fn build(b: &BoundShape<HipFunction, f32>, settings: &Settings) -> Option<Self> {
        let f = b.shape().inner();
        let tape = f.tape();
        let m = settings.world_to_model.transpose();
        let axes = axis_slots(fidget_core::eval::Function::vars(f));
        let (keys, vals): (Vec<u64>, Vec<f32>) = b.vars().iter().map(|(k, v)| (var_key(*k), *v)).unzip();
        let mut h = std::ptr::null_mut();
        let st = CTX.with(|c| unsafe {
            let name = b"mesh_keep_device\0";
            ffi::fhip_ctx_set_option(c.raw(), name.as_ptr().cast(), 1);
            let st = ffi::fhip_mesh_build(c.raw(), tape.raw(), settings.depth as u32, m.as_ptr(), axes.as_ptr(), keys.as_ptr(), vals.as_ptr(),
                                          keys.len() as u32, &mut h);
            ffi::fhip_ctx_set_option(c.raw(), name.as_ptr().cast(), 0);
            st
        });
        if st != 0 { None } else { Some(DeviceMesh { h }) }
    }

    /// `Mesh::write_stl`: the same bytes, packed on the device (`fhip_mesh_stl`)
    pub fn write_stl<F: std::io::Write>(&self, out: &mut F) -> std::io::Result<()> {
        let mut bytes = vec![0u8; unsafe { ffi::fhip_mesh_stl_bytes(self.h) } as usize];
        let st = CTX.with(|c| unsafe { ffi::fhip_mesh_stl(c.raw(), self.h, bytes.as_mut_ptr().cast(), 0) });
        if st != 0 {
            return Err(std::io::Error::new(std::io::ErrorKind::Other, format!("fhip_mesh_stl: status {st}")));
        }
        out.write_all(&bytes)
    }

    /// `Grad {v, dx, dy, dz}` of `b` at every vertex (`fhip_mesh_vertex_grads`): model space, not normalised
    pub fn vertex_grads(&self, b: &BoundShape<HipFunction, f32>) -> Option<Vec<[f32; 4]>> {
        let f = b.shape().inner();
        let axes = axis_slots(fidget_core::eval::Function::vars(f));
        let (keys, vals): (Vec<u64>, Vec<f32>) = b.vars().iter().map(|(k, v)| (var_key(*k), *v)).unzip();
        let mut n = [0u64; 8];
        unsafe { ffi::fhip_mesh_counts(self.h, n.as_mut_ptr()) };
        let mut out = vec![[0f32; 4]; n[6] as usize];
        let st = CTX.with(|c| unsafe {
            ffi::fhip_mesh_vertex_grads(c.raw(), f.tape().raw(), self.h, axes.as_ptr(), keys.as_ptr(), vals.as_ptr(), keys.len() as u32,
                                        out.as_mut_ptr().cast(), 0)
        });
        if st != 0 { None } else { Some(out) }
    }
}

impl Drop for DeviceMesh {
    fn drop(&mut self) {
        unsafe { ffi::fhip_mesh_free(self.h) };
    }
}
