//! Connected components of a voxel bitmap (`fhip_voxels_components`): is the solid one body or several, and does it enclose voids.  The
//! foreground is the set bits of a `Voxels`, or with `complement` its clear bits; neighbours share a face (connectivity 6) or a face, an
//! edge or a corner (26).  Components are numbered by ascending seed - their voxel of smallest key `word * 64 + bit`.
use std::os::raw::c_void;

use crate::voxels::Voxels;
use crate::{ffi, CTX};

/// The table of a labelling, on the host; the handle keeps the per-brick arrays on the device until it is dropped
pub struct Components<'a> {
    voxels: &'a Voxels,
    handle: *mut c_void,
    /// The bricks' own components, which the union-find joined
    pub nodes: u64,
    /// Foreground voxels
    pub voxel_count: u64,
    /// Voxels per component
    pub sizes: Vec<u64>,
    /// `[i, j, k]` of every component's seed
    pub seeds: Vec<[u32; 3]>,
    /// Inclusive bounds per axis
    pub lo: Vec<[u32; 3]>,
    pub hi: Vec<[u32; 3]>,
    /// Whether the component touches the grid's border (with `complement`: the others are enclosed voids)
    pub border: Vec<bool>,
}

impl Drop for Components<'_> {
    fn drop(&mut self) {
        unsafe { ffi::fhip_components_free(self.handle) }
    }
}

impl Components<'_> {
    /// The number of components
    pub fn count(&self) -> usize {
        self.sizes.len()
    }
    /// The largest component (of several, the one of smallest id)
    pub fn largest(&self) -> Option<usize> {
        (0..self.count()).rev().max_by_key(|&k| self.sizes[k])
    }
    /// Label images for `k0 <= k < k1`: `[(k - k0) * N + j] * N + i` = the component of voxel `(i, j, k)`, -1 for background
    pub fn label_slices(&self, k0: u32, k1: u32) -> Option<Vec<i32>> {
        let n = self.voxels.grid();
        let mut out = vec![0i32; (k1.saturating_sub(k0)) as usize * n * n];
        let st = CTX.with(|c| unsafe {
            ffi::fhip_components_label_slices(c.raw(), self.handle, self.voxels.bricks.as_ptr(), 0, k0, k1, out.as_mut_ptr(), 0)
        });
        if st != 0 { None } else { Some(out) }
    }
    /// The components `ids` as a bitmap of their own
    pub fn extract(&self, ids: &[u32]) -> Option<Voxels> {
        let mut bricks = vec![0u64; self.voxels.bricks.len()];
        let st = CTX.with(|c| unsafe {
            ffi::fhip_components_extract(c.raw(), self.handle, self.voxels.bricks.as_ptr(), 0, ids.as_ptr(), ids.len() as u64, bricks.as_mut_ptr(), 0)
        });
        if st != 0 { None } else { Some(Voxels { bricks, depth: self.voxels.depth, cells: [0; 4] }) }
    }
}

/// The components of `voxels` under `connectivity` (6 or 26); `None` when the call is refused
pub fn components(voxels: &Voxels, connectivity: u32, complement: bool) -> Option<Components<'_>> {
    let mut handle: *mut c_void = std::ptr::null_mut();
    let st = CTX.with(|c| unsafe {
        ffi::fhip_voxels_components(c.raw(), voxels.bricks.as_ptr(), voxels.depth, 0, connectivity, complement as i32, &mut handle)
    });
    if st != 0 {
        return None;
    }
    let mut counts = [0u64; 4];
    unsafe { ffi::fhip_components_counts(handle, counts.as_mut_ptr()) };
    let n = counts[0] as usize;
    let (mut sizes, mut seeds, mut lo, mut hi, mut border) = (vec![0u64; n], vec![[0u32; 3]; n], vec![[0u32; 3]; n], vec![[0u32; 3]; n], vec![0u8; n]);
    let st = unsafe {
        ffi::fhip_components_table(handle, sizes.as_mut_ptr(), seeds.as_mut_ptr().cast(), lo.as_mut_ptr().cast(), hi.as_mut_ptr().cast(), border.as_mut_ptr())
    };
    let c = Components { voxels, handle, nodes: counts[1], voxel_count: counts[2], sizes, seeds, lo, hi, border: border.iter().map(|&b| b != 0).collect() };
    if st != 0 { None } else { Some(c) }
}
