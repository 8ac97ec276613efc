//! Shape voxels (`fhip_shape_voxels`): the inside voxels of the grid `occupancy` counts, written down as a bitmap - one `u64` per brick
//! of 4 x 4 x 4 voxels, `B^3` of them with `B = 1 << depth`.  Word `(bz * B + by) * B + bx` is the brick of the voxels
//! `(4 bx + lx, 4 by + ly, 4 bz + lz)`, bit `lx + 4 ly + 16 lz` set iff that voxel is inside.  Layer images and voxels per layer are
//! made of the bitmap on the device (`fhip_voxels_slices`, `fhip_voxels_layer_counts`).
use fidget_core::shape::BoundShape;
use fidget_mesh::Settings;

use crate::{axis_slots, ffi, var_key, HipFunction, CTX};

/// A bitmap on the host, with the octree's counters `[cells evaluated, Full, Empty, ambiguous cells of the last level]`
#[derive(Clone, Debug, PartialEq, Eq)]
pub struct Voxels {
    pub bricks: Vec<u64>,
    pub depth: u32,
    pub cells: [u64; 4],
}

impl Voxels {
    /// Voxels per axis
    pub fn grid(&self) -> usize {
        4usize << self.depth
    }
    /// The number of inside voxels
    pub fn count(&self) -> u64 {
        self.bricks.iter().map(|w| w.count_ones() as u64).sum()
    }
    /// Whether voxel `(i, j, k)` is inside
    pub fn get(&self, i: usize, j: usize, k: usize) -> bool {
        let b = 1usize << self.depth;
        let word = self.bricks[((k / 4) * b + j / 4) * b + i / 4];
        (word >> ((i % 4) + 4 * (j % 4) + 16 * (k % 4))) & 1 != 0
    }
    /// Layer images for `k0 <= k < k1`: `(k1 - k0) * N * N` bytes, `[(k - k0) * N + j] * N + i` = 255 inside, 0 outside; `None` when refused
    pub fn slices(&self, k0: u32, k1: u32) -> Option<Vec<u8>> {
        let n = self.grid();
        let mut out = vec![0u8; (k1.saturating_sub(k0)) as usize * n * n];
        let st = CTX.with(|c| unsafe { ffi::fhip_voxels_slices(c.raw(), self.bricks.as_ptr(), self.depth, k0, k1, out.as_mut_ptr(), 0) });
        if st != 0 { None } else { Some(out) }
    }
    /// Inside voxels per third index `k`; `None` when refused
    pub fn layer_counts(&self) -> Option<Vec<u64>> {
        let mut out = vec![0u64; self.grid()];
        let st = CTX.with(|c| unsafe { ffi::fhip_voxels_layer_counts(c.raw(), self.bricks.as_ptr(), self.depth, out.as_mut_ptr(), 0) });
        if st != 0 { None } else { Some(out) }
    }
}

/// The bitmap of `shape` at `settings.depth` (at most 10) under `settings.world_to_model`; `None` when the variables do not bind or the
/// call is refused
pub fn voxelize(b: &BoundShape<HipFunction, f32>, settings: &Settings) -> Option<Voxels> {
    let f = b.shape().inner();
    let m = settings.world_to_model.transpose();
    let axes = axis_slots(fidget_core::eval::Function::vars(f));
    let (keys, vals): (Vec<u64>, Vec<f32>) = b.vars().iter().map(|(k, v)| (var_key(*k), *v)).unzip();
    let depth = settings.depth as u32;
    let words = unsafe { ffi::fhip_voxels_words(depth) } as usize;
    if words == 0 {
        return None;
    }
    let mut bricks = vec![0u64; words];
    let mut cells = [0u64; 4];
    let st = CTX.with(|c| unsafe {
        ffi::fhip_shape_voxels(c.raw(), f.tape().raw(), depth, m.as_ptr(), axes.as_ptr(), keys.as_ptr(), vals.as_ptr(), keys.len() as u32,
                               bricks.as_mut_ptr(), 0, cells.as_mut_ptr())
    });
    if st != 0 { None } else { Some(Voxels { bricks, depth, cells }) }
}

/// What a mesh's voxelization reports: `[triangles, rejected, flat, crossings, clipped, open_rows, set voxels, W]`; `open_rows > 0`
/// shows a mesh that is not closed
pub type MeshInfo = [u64; 8];

/// The solid a closed triangle mesh encloses (`fhip_triangles_voxels`: parity counting along +x, exact in integers after the vertices
/// are snapped to 1/256 voxel) on the grid of `4 << depth` voxels per axis over `[-1, 1]^3`.  `triangles`: vertex indices, or `None`
/// for a soup in which every three vertices are a triangle; `mesh_to_world`: a row-major 3 x 4 matrix.  The bitmap's `cells` are zeros.
/// `None` when the call is refused.
pub fn voxelize_triangles(vertices: &[[f32; 3]], triangles: Option<&[[u64; 3]]>, mesh_to_world: Option<&[f64; 12]>, depth: u32) -> Option<(Voxels, MeshInfo)> {
    let words = unsafe { ffi::fhip_voxels_words(depth) } as usize;
    if words == 0 {
        return None;
    }
    let mut bricks = vec![0u64; words];
    let mut info = [0u64; 8];
    let n_triangles = triangles.map_or(vertices.len() / 3, |t| t.len()) as u64;
    let st = CTX.with(|c| unsafe {
        ffi::fhip_triangles_voxels(c.raw(), vertices.as_ptr() as *const f32, vertices.len() as u64, triangles.map_or(std::ptr::null(), |t| t.as_ptr() as *const u64),
                                   n_triangles, 0, mesh_to_world.map_or(std::ptr::null(), |m| m.as_ptr()), depth, bricks.as_mut_ptr(), 0, info.as_mut_ptr())
    });
    if st != 0 { None } else { Some((Voxels { bricks, depth, cells: [0; 4] }, info)) }
}

/// The same for a mesh the library built (`fhip_mesh_voxels`), read from its device arrays where they are resident.
///
/// # Safety
/// `mesh` must be a live `fhip_mesh` of this library.
pub unsafe fn voxelize_built_mesh(mesh: *const ffi::fhip_mesh, mesh_to_world: Option<&[f64; 12]>, depth: u32) -> Option<(Voxels, MeshInfo)> {
    let words = ffi::fhip_voxels_words(depth) as usize;
    if words == 0 {
        return None;
    }
    let mut bricks = vec![0u64; words];
    let mut info = [0u64; 8];
    let st = CTX.with(|c| ffi::fhip_mesh_voxels(c.raw(), mesh, mesh_to_world.map_or(std::ptr::null(), |m| m.as_ptr()), depth, bricks.as_mut_ptr(), 0, info.as_mut_ptr()));
    if st != 0 { None } else { Some((Voxels { bricks, depth, cells: [0; 4] }, info)) }
}
