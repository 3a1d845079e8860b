//! src/render_gpu.rs — what replaces the thread fan-out of `render()` in the reference (src/main.rs:275-303: spawn,
//! render_pixel per pixel, put_pixel under the mutex, recv).  Everything before it (pixel list aside: it is not needed
//! any more) and after it (timing print, PNG write, src/main.rs:305-315) stays as it is.
//!
//! Call sequence = the one ray-tracer-rust_amd/host/tracer.hpp (C++, tested) makes:
//!   flatten the Vec<Primitive> (before BoundingVolumeHierarchy::new consumes it, src/main.rs:357)
//!   -> rtx_scene_create -> rtx_render_frame over every device -> rtx_scene_destroy.
//!
//! A moving light: `render_frame` below bakes `light` into the scene it creates, which is what the render pipeline reads.
//! A caller that keeps the scene handle and wants the same geometry under another light, or at another NB_LIGHT_SAMPLE,
//! does not create a scene per light: `rtx_ffi::rtx_render_view_lit` (any view of the scene) and
//! `rtx_ffi::rtx_shade_rays_lit` (the caller's rays) take an `rtx_ffi::RtxLight` — the triangle's three vertices as
//! `light_v0..2` are filled here, and the count — per call; `rtx_ffi::rtx_scene_light` reads the scene's own back
//!.
use rtx_ffi::{self, RtxScene, RtxSceneDesc, RtxStats, Sample};
use std::ptr;
use tracer::primitives::Primitive;
use tracer::utils::camera::Camera;
use tracer::utils::color::Color;

/// The primitives as the library takes them: built in `main()` from the same Vec that goes into the BVH.
pub struct FlatScene {
    pub v0v1v2: Vec<f32>,    // 9 per triangle
    pub rgb: Vec<f32>,       // 3 per triangle
    pub spheres: Vec<f32>,   // 4 per sphere: origin, radius
    pub sphere_rgb: Vec<f32>,
    pub kinds: Vec<u8>,      // Vec order: 0 = next triangle, 1 = next sphere
}

pub fn flatten(primitives: &[Primitive]) -> FlatScene {
    let mut f = FlatScene { v0v1v2: Vec::new(), rgb: Vec::new(), spheres: Vec::new(), sphere_rgb: Vec::new(), kinds: Vec::new() };
    for p in primitives {
        match p {
            &Primitive::Triangle(ref t) => {
                f.v0v1v2.extend_from_slice(&[t.v0.x, t.v0.y, t.v0.z, t.v1.x, t.v1.y, t.v1.z, t.v2.x, t.v2.y, t.v2.z]);
                f.rgb.extend_from_slice(&[t.color.red, t.color.green, t.color.blue]);
                f.kinds.push(0);
            }
            &Primitive::Sphere(ref s) => {
                f.spheres.extend_from_slice(&[s.origin.x, s.origin.y, s.origin.z, s.radius]);
                f.sphere_rgb.extend_from_slice(&[s.color.red, s.color.green, s.color.blue]);
                f.kinds.push(1);
            }
        }
    }
    f
}

/// RGB8 rows of the whole frame, `rgb[(py * width + px) * 3 ..]` = what `put_pixel(px, py, color.to_rgba())` stored
/// (src/main.rs:293-294).  `samples` is the table of src/main.rs:253 as `Vec<Sample>` (see rtx_ffi::Sample).
pub fn render_frame(width: u32, height: u32, camera: &Camera, light: &Primitive, flat: &FlatScene, samples: &[Sample],
                    nb_ray: u32, nb_light_sample: u32) -> Result<(Vec<u8>, RtxStats), String> {
    let lt = match light {
        &Primitive::Triangle(ref t) => t,
        _ => return Err("the light must be a triangle (light.rs:11-13 samples primitives[0])".to_string()),
    };
    let (u, v, w) = (camera.u.as_ref(), camera.v.as_ref(), camera.w.as_ref());
    let null_if_empty = |x: &Vec<f32>| if x.is_empty() { ptr::null() } else { x.as_ptr() };
    let desc = RtxSceneDesc {
        width: width,
        height: height,
        eye: [camera.eye.x, camera.eye.y, camera.eye.z],
        u: [u.x, u.y, u.z],
        v: [v.x, v.y, v.z],
        w: [w.x, w.y, w.z],
        distance: camera.distance,
        light_v0: [lt.v0.x, lt.v0.y, lt.v0.z],
        light_v1: [lt.v1.x, lt.v1.y, lt.v1.z],
        light_v2: [lt.v2.x, lt.v2.y, lt.v2.z],
        n_tris: (flat.rgb.len() / 3) as u32,
        v0v1v2: null_if_empty(&flat.v0v1v2),
        rgb: null_if_empty(&flat.rgb),
        tie_rank: ptr::null(),              // the library rebuilds the reference tree for exact ties (reference_tree: 0)
        nb_ray: nb_ray,
        nb_light_sample: nb_light_sample,
        samples: samples.as_ptr() as *const f32,
        n_samples: samples.len() as u32,
        accel: 0,
        leaf_max: 0,
        reference_tree: 0,
        n_spheres: (flat.sphere_rgb.len() / 3) as u32,
        spheres: null_if_empty(&flat.spheres),
        sphere_rgb: null_if_empty(&flat.sphere_rgb),
        kinds: flat.kinds.as_ptr(),
    };
    let mut handle: *mut RtxScene = ptr::null_mut();
    let mut rgb = vec![0u8; (width as usize) * (height as usize) * 3];
    let mut stats = RtxStats::default();
    let devices: Vec<i32> = (0..unsafe { rtx_ffi::rtx_device_count() }).collect();
    if devices.is_empty() {
        return Err("librtx: no HIP device (there is no CPU fallback)".to_string());
    }
    unsafe {
        rtx_ffi::check(rtx_ffi::rtx_scene_create(&desc, &mut handle))?;
        let rc = rtx_ffi::rtx_render_frame(handle, devices.as_ptr(), devices.len() as i32, 8, rgb.as_mut_ptr(), &mut stats);
        rtx_ffi::rtx_scene_destroy(handle);
        rtx_ffi::check(rc)?;
    }
    let _ = Color::new_black();              // (Color stays the crate's type for everything outside this call)
    Ok((rgb, stats))
}
