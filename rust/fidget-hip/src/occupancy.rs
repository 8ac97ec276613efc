//! Shape occupancy (`fhip_shape_occupancy`): how big a solid is, where its centre of mass lies and what box it fits in, from exact integer
//! sums over the inside voxels of a regular grid of `4 << depth` per axis over `[-1, 1]^3` - counted down the mesher's octree, so only
//! the cells the surface passes through are sampled.
use fidget_core::shape::BoundShape;
use fidget_mesh::Settings;

use crate::{axis_slots, ffi, var_key, HipFunction, CTX};

/// The integers of the result, and what follows from them in `f64` in the region's own coordinates (`h = 2 / grid`)
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct Occupancy(pub ffi::fhip_occupancy);

impl Occupancy {
    pub fn h(&self) -> f64 {
        2.0 / self.0.grid as f64
    }
    pub fn volume(&self) -> f64 {
        self.0.n as f64 * self.h().powi(3)
    }
    /// Mean of the inside voxels' centres; `None` for an empty shape
    pub fn centroid(&self) -> Option<[f64; 3]> {
        if self.0.n == 0 {
            return None;
        }
        let (n, h) = (self.0.n as f64, self.h());
        Some([0, 1, 2].map(|k| -1.0 + (self.0.s1[k] as f64 / n + 0.5) * h))
    }
    /// The faces of the outermost inside voxels, `(min, max)`; `None` for an empty shape
    pub fn bounds(&self) -> Option<([f64; 3], [f64; 3])> {
        if self.0.n == 0 {
            return None;
        }
        let h = self.h();
        Some(([0, 1, 2].map(|k| -1.0 + self.0.lo[k] as f64 * h), [0, 1, 2].map(|k| -1.0 + (self.0.hi[k] + 1) as f64 * h)))
    }
}

/// Occupancy of `shape` at `settings.depth` (at most 10) under `settings.world_to_model`; `None` when the variables do not bind or the
/// call is refused
pub fn occupancy(b: &BoundShape<HipFunction, f32>, settings: &Settings) -> Option<Occupancy> {
    let f = b.shape().inner();
    let m = settings.world_to_model.transpose();
    let axes = axis_slots(fidget_core::eval::Function::vars(f));
    let (keys, vals): (Vec<u64>, Vec<f32>) = b.vars().iter().map(|(k, v)| (var_key(*k), *v)).unzip();
    let mut out = ffi::fhip_occupancy::default();
    let st = CTX.with(|c| unsafe {
        ffi::fhip_shape_occupancy(c.raw(), f.tape().raw(), settings.depth as u32, m.as_ptr(), axes.as_ptr(), keys.as_ptr(), vals.as_ptr(),
                                  keys.len() as u32, (&mut out as *mut ffi::fhip_occupancy).cast())
    });
    if st != 0 { None } else { Some(Occupancy(out)) }
}
