"""A light stage without Blender: cameras and point lights on a Fibonacci sphere around a target, as the cam.json / light.json
dicts the rest of data_gen reads.  Deterministic: no random numbers."""
import numpy as np

GOLDEN_ANGLE = np.pi * (3.0 - np.sqrt(5.0))


def fibonacci_sphere(n, hemisphere=False, phase=0.0):
    """n unit vectors [n,3]: z = 1 - (2k + 1) / n over the sphere (hemisphere: z = 1 - (k + 1/2) / n, the upper half), azimuth
    k * the golden angle + phase."""
    k = np.arange(int(n), dtype=np.float64)
    z = 1.0 - (k + 0.5) / n if hemisphere else 1.0 - (2.0 * k + 1.0) / n
    r = np.sqrt(1.0 - z * z)
    phi = k * GOLDEN_ANGLE + phase
    return np.stack((r * np.cos(phi), r * np.sin(phi), z), 1)


def look_at_euler(position, target, up=(0.0, 0.0, 1.0)):
    """Blender 'XYZ' Euler angles (radians) of a camera at `position` looking at `target` down its -z axis with y up: the inverse
    of `mesh.euler_xyz_matrix` for the look-at rotation.  Looking straight along `up`, the x axis is used as the up vector."""
    position, target = np.asarray(position, np.float64), np.asarray(target, np.float64)
    z = position - target
    z = z / np.linalg.norm(z)
    x = np.cross(np.asarray(up, np.float64), z)
    if np.linalg.norm(x) < 1e-9:
        x = np.cross(np.array([1.0, 0.0, 0.0]), z)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    r = np.stack((x, y, z), 1)                                      # camera -> world = Rz . Ry . Rx
    # x is perpendicular to `up` or to the x axis, so r[2, 0] = 0 for the default `up`: no gimbal lock
    ry = -np.arcsin(np.clip(r[2, 0], -1.0, 1.0))
    return [float(np.arctan2(r[2, 1], r[2, 2])), float(ry), float(np.arctan2(r[1, 0], r[0, 0]))]


def light_stage(n_cams, n_lights, radius, target, focal_length=50.0, sensor=(32.0, 24.0), hemisphere=False, light_radius=None,
                cam_prefix='C', light_prefix='L', phase=0.0, light_size=0.1):
    """-> (cams, lights): lists of dicts with the reference's key sets -- name, position, rotation, focal_length, sensor_width,
    sensor_height, clip_start, clip_end / name, position, size -- `n_cams` cameras at `radius` from `target` looking at it, and
    `n_lights` lights at `light_radius` (default: `radius`), both on Fibonacci spheres (the lights' azimuths turned by half a
    golden angle so that a light never sits in a camera).  hemisphere: the upper (z > target.z) half only.  phase turns the whole
    rig about z: another phase gives held-out positions.  Names are prefix + a zero-padded index.  `light_size` is the radius Blender gives a point lamp: nlt_render_direct's
    lights are points and ignore it, `shade.render_global` samples a sphere of that radius."""
    target = np.asarray(target, np.float64).reshape(3)
    light_radius = radius if light_radius is None else light_radius
    cams, lights = [], []
    for k, p in enumerate(fibonacci_sphere(n_cams, hemisphere, phase)):
        pos = target + radius * p
        cams.append(dict(name='%s%03d' % (cam_prefix, k), position=[float(x) for x in pos], rotation=look_at_euler(pos, target),
                         focal_length=float(focal_length), sensor_width=float(sensor[0]), sensor_height=float(sensor[1]),
                         clip_start=0.1, clip_end=float(max(100.0, 10.0 * radius))))
    for k, p in enumerate(fibonacci_sphere(n_lights, hemisphere, phase + 0.5 * GOLDEN_ANGLE)):
        lights.append(dict(name='%s%03d' % (light_prefix, k), position=[float(x) for x in target + light_radius * p],
                           size=float(light_size)))
    return cams, lights
