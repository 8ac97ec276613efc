//! The check of a triangle mesh (`fhip_triangles_topology`): the welded indexed mesh, the class of every edge - boundary, flipped,
//! nonmanifold, unbalanced - and the shells, the edge-connected parts, with their triangles, bounds, volume and area.  Every integer is
//! the same from run to run; `volume6` and `area2` are float64 sums of the same terms in an order of arrival that may differ, and
//! they alone.  The definitions stand in `include/fidget_hip.h`.
use std::os::raw::c_void;

use crate::{ffi, CTX};

/// The classes of `Topology::edges`
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum EdgeKind {
    Boundary = 0,
    Flipped = 1,
    Nonmanifold = 2,
    Unbalanced = 3,
}

/// One shell, numbered in the order of the shells' first triangles; `volume6 < 0`: an inward-facing cavity
#[derive(Clone, Debug, PartialEq)]
pub struct Shell {
    pub triangles: u64,
    pub first: u32,
    pub unbalanced: u64,
    pub lo: [f32; 3],
    pub hi: [f32; 3],
    pub volume6: f64,
    pub area2: f64,
}

/// What the check found, on the host; the handle keeps the arrays on the device until it is dropped
pub struct Topology {
    handle: *mut c_void,
    /// triangles, rejected, degenerate, vertices, edges, boundary, flipped, nonmanifold, unbalanced, shells, vertex slots, edge slots
    pub counts: [u64; 16],
    pub shells: Vec<Shell>,
}

impl Drop for Topology {
    fn drop(&mut self) {
        unsafe { ffi::fhip_topology_free(self.handle) }
    }
}

impl Topology {
    /// No unbalanced edge: the triangles form a cycle, what parity filling needs
    pub fn closed(&self) -> bool {
        self.counts[8] == 0
    }
    /// No boundary, flipped or nonmanifold edge
    pub fn manifold(&self) -> bool {
        self.counts[5] == 0 && self.counts[6] == 0 && self.counts[7] == 0
    }
    /// vertices - edges + (triangles - degenerate)
    pub fn euler(&self) -> i64 {
        self.counts[3] as i64 - self.counts[4] as i64 + self.counts[0] as i64 - self.counts[2] as i64
    }
    pub fn volume(&self) -> f64 {
        self.shells.iter().map(|s| s.volume6).sum::<f64>() / 6.0
    }
    pub fn area(&self) -> f64 {
        self.shells.iter().map(|s| s.area2).sum::<f64>() / 2.0
    }
    /// The vertices: welded, in the order of their first corners, or as given
    pub fn vertices(&self) -> Option<Vec<[f32; 3]>> {
        let mut out = vec![[0f32; 3]; unsafe { ffi::fhip_topology_vertex_rows(self.handle) } as usize];
        let st = unsafe { ffi::fhip_topology_vertices(self.handle, out.as_mut_ptr().cast()) };
        if st != 0 { None } else { Some(out) }
    }
    /// Every triangle in the order given, as vertex ids
    pub fn triangles(&self) -> Option<Vec<[u64; 3]>> {
        let mut out = vec![[0u64; 3]; if self.counts[1] != 0 { 0 } else { self.counts[0] as usize }];
        let st = unsafe { ffi::fhip_topology_triangles(self.handle, out.as_mut_ptr().cast()) };
        if st != 0 { None } else { Some(out) }
    }
    /// A shell per triangle, `0xFFFFFFFF` for a degenerate one
    pub fn triangle_shells(&self) -> Option<Vec<u32>> {
        let mut out = vec![0u32; if self.counts[1] != 0 { 0 } else { self.counts[0] as usize }];
        let st = unsafe { ffi::fhip_topology_triangle_shells(self.handle, out.as_mut_ptr()) };
        if st != 0 { None } else { Some(out) }
    }
    /// The edges of one class as vertex pairs `(a, b)`, `a < b`, in the order of the first corners that use them
    pub fn edges(&self, kind: EdgeKind) -> Option<Vec<[u32; 2]>> {
        let mut out = vec![[0u32; 2]; self.counts[5 + kind as usize] as usize];
        let st = CTX.with(|c| unsafe { ffi::fhip_topology_edges(c.raw(), self.handle, kind as u32, out.as_mut_ptr().cast(), 0) });
        if st != 0 { None } else { Some(out) }
    }
}

/// The check of a mesh on the host.  `triangles`: vertex indices, or `None` for a soup in which every three vertices are a triangle and
/// which is always welded; `weld`: make one vertex of all corners with equal coordinates.  `None` when the call is refused; a result
/// with `counts[1] != 0` holds rejected triangles and nothing else.
pub fn topology(vertices: &[[f32; 3]], triangles: Option<&[[u64; 3]]>, weld: bool) -> Option<Topology> {
    let n_triangles = triangles.map_or(vertices.len() as u64 / 3, |t| t.len() as u64);
    let mut handle: *mut c_void = std::ptr::null_mut();
    let st = CTX.with(|c| unsafe {
        ffi::fhip_triangles_topology(c.raw(), vertices.as_ptr() as *const f32, vertices.len() as u64, triangles.map_or(std::ptr::null(), |t| t.as_ptr() as *const u64),
                                     n_triangles, 0, (weld || triangles.is_none()) as i32, 0, &mut handle)
    });
    if st != 0 {
        return None;
    }
    let mut counts = [0u64; 16];
    unsafe { ffi::fhip_topology_counts(handle, counts.as_mut_ptr()) };
    let n = counts[9] as usize;
    let (mut tri, mut first, mut unb, mut lo, mut hi, mut v6, mut a2) = (vec![0u64; n], vec![0u32; n], vec![0u64; n], vec![[0f32; 3]; n], vec![[0f32; 3]; n], vec![0f64; n], vec![0f64; n]);
    let st = unsafe {
        ffi::fhip_topology_shells(handle, tri.as_mut_ptr(), first.as_mut_ptr(), unb.as_mut_ptr(), lo.as_mut_ptr().cast(), hi.as_mut_ptr().cast(), v6.as_mut_ptr(), a2.as_mut_ptr())
    };
    let shells = (0..n).map(|k| Shell { triangles: tri[k], first: first[k], unbalanced: unb[k], lo: lo[k], hi: hi[k], volume6: v6[k], area2: a2[k] }).collect();
    let t = Topology { handle, counts, shells };
    if st != 0 { None } else { Some(t) }
}
