//! Contours of a 2D slice (`fhip_contour2d`): the outlines of `shape < 0` in the pixel-perfect `render2d` image of a configuration, by
//! marching squares on the device - a vertex on every lattice edge whose ends differ, directed segments with the inside on their left,
//! and the link array `next` that `loops` follows.  Coordinates are pixel units: the centre of pixel `(i, j)` is `(i as f32, j as f32)`.
use std::os::raw::c_void;

use fidget_core::shape::BoundShape;
use fidget_raster::pixel;

use crate::{axis_slots, ffi, var_key, HipFunction, CTX};

/// The arrays of a result, copied to the host
#[derive(Clone, Debug, PartialEq)]
pub struct Contours {
    /// `[x, y]` in pixel units, one per crossing lattice edge in edge-index order
    pub vertices: Vec<[f32; 2]>,
    /// `[from, to]` vertex ids, in cell order
    pub segments: Vec<[u32; 2]>,
    /// `next[k]`: where the segment leaving vertex `k` goes; `u32::MAX` when none does (only on the image's border)
    pub next: Vec<u32>,
    /// Image width in pixels
    pub width: u32,
    /// Image height in pixels
    pub height: u32,
}

impl Contours {
    /// The chains of `next` as `(ids, closed)`: open chains first, then closed loops, each from its smallest id (`fhip_contour_loops`)
    pub fn loops(&self) -> Option<Vec<(Vec<u32>, bool)>> {
        let n = self.next.len();
        let (mut order, mut start, mut closed, mut count) = (vec![0u32; n], vec![0u64; n + 1], vec![0u8; n], 0u64);
        let st = unsafe {
            ffi::fhip_contour_loops(self.next.as_ptr(), n as u64, order.as_mut_ptr(), start.as_mut_ptr(), closed.as_mut_ptr(), &mut count)
        };
        if st != 0 {
            return None;
        }
        Some((0..count as usize).map(|k| (order[start[k] as usize..start[k + 1] as usize].to_vec(), closed[k] != 0)).collect())
    }
    /// Signed area of a chain in pixel units (shoelace sum in `f64`): positive for an outer boundary, negative for a hole
    pub fn area(&self, ids: &[u32]) -> f64 {
        let p = |k: usize| (self.vertices[ids[k] as usize][0] as f64, self.vertices[ids[k] as usize][1] as f64);
        0.5 * (0..ids.len()).map(|k| { let (a, b) = (p(k), p((k + 1) % ids.len())); a.0 * b.1 - b.0 * a.1 }).sum::<f64>()
    }
}

/// The contours of `shape` under `cfg` (its `pixel_perfect` is taken as set); `None` when the variables do not bind or the call is refused
pub fn contour(b: &BoundShape<HipFunction, f32>, cfg: &pixel::RenderConfig) -> Option<Contours> {
    let f = b.shape().inner();
    let m = cfg.world_to_model.transpose();
    let axes = axis_slots(fidget_core::eval::Function::vars(f));
    let (keys, vals): (Vec<u64>, Vec<f32>) = b.vars().iter().map(|(k, v)| (var_key(*k), *v)).unzip();
    let c = ffi::fhip_render2d_config {
        width: cfg.image_size.width(),
        height: cfg.image_size.height(),
        world_to_model: m.as_ptr(),
        z: cfg.z,
        pixel_perfect: 1,
        tile_sizes: std::ptr::null(),
        n_tile_sizes: 0,
        var_keys: keys.as_ptr(),
        var_values: vals.as_ptr(),
        n_vars: keys.len() as u32,
        axis_slots: axes.as_ptr(),
    };
    let mut h: *mut c_void = std::ptr::null_mut();
    let st = CTX.with(|ctx| unsafe { ffi::fhip_contour2d(ctx.raw(), f.tape().raw(), &c, &mut h) });
    if st != 0 {
        return None;
    }
    let mut counts = [0u64; 4];
    unsafe { ffi::fhip_contours_counts(h, counts.as_mut_ptr()) };
    let (nv, ns) = (counts[0] as usize, counts[1] as usize);
    let (mut vertices, mut segments, mut next) = (vec![[0f32; 2]; nv], vec![[0u32; 2]; ns], vec![0u32; nv]);
    let ok = unsafe {
        let st_vertices = ffi::fhip_contours_vertices(h, vertices.as_mut_ptr().cast());
        let st_segments = ffi::fhip_contours_segments(h, segments.as_mut_ptr().cast());
        let st_next = ffi::fhip_contours_next(h, next.as_mut_ptr());
        ffi::fhip_contours_free(h);
        st_vertices == 0 && st_segments == 0 && st_next == 0
    };
    if ok { Some(Contours { vertices, segments, next, width: c.width, height: c.height }) } else { None }
}
