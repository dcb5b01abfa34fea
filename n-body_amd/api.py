"""Host-side mirror of the reference's C++ interface for the hot path, over the C ABI.

Names, argument meaning and error behaviour follow the reference headers so that the parity
tests read like the reference's own tests:

  ParticleData / ParticleDataManager    include/nbody/types.hpp:234-276, particle_data.hpp:9-36
  ForceCalculator / DirectForceCalculator / createForceCalculator
                                        include/nbody/force_calculator.hpp:36-231
  Integrator                            include/nbody/integrator.hpp:51-150
  SimulationConfig / ForceMethod        include/nbody/types.hpp:66-101,301-313
  validate*                             src/utils/error_handling.cpp:46-123

PyTorch is used only as the owner of device memory and of the HIP stream; every computation is
a call into libnbody_hip.so.  The compiled-language facade (C++) lives in n-body_amd/facade/.
"""
from __future__ import annotations

import ctypes as C
import enum
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import (FIELDS, ParticleDataStruct, StateException, ValidationException, check)


class ForceMethod(enum.IntEnum):  # types.hpp:66-70
    DIRECT_N2 = 0
    BARNES_HUT = 1
    SPATIAL_HASH = 2


class InitDistribution(enum.IntEnum):  # types.hpp:82-86
    UNIFORM = 0
    SPHERICAL = 1
    DISK = 2


@dataclass
class SimulationConfig:  # types.hpp:301-313 (same defaults)
    particle_count: int = 10000
    init_distribution: InitDistribution = InitDistribution.SPHERICAL
    force_method: ForceMethod = ForceMethod.DIRECT_N2
    dt: float = 0.001
    G: float = 1.0
    softening: float = 0.1
    barnes_hut_theta: float = 0.5
    spatial_hash_cell_size: float = 1.0
    spatial_hash_cutoff: float = 2.0
    cuda_block_size: int = 256


# ---- validators (error_handling.cpp:46-123; same messages) ------------------------------------

def _finite(v):
    return not (math.isnan(v) or math.isinf(v))


def validateParticleCountRange(count):
    if count == 0:
        raise ValidationException("Particle count must be greater than 0")
    if count > 100000000:
        raise ValidationException("Particle count exceeds maximum supported (100M)")


def validateTimeStep(dt):  # same check order as error_handling.cpp:91-103
    if dt <= 0:
        raise ValidationException("Time step must be positive")
    if math.isnan(dt) or math.isinf(dt):
        raise ValidationException("Time step must be a finite number")
    if dt > 1.0:
        raise ValidationException("Time step is too large (max 1.0)")


def validateSoftening(eps):  # error_handling.cpp:105-113
    if eps < 0:
        raise ValidationException("Softening parameter must be non-negative")
    if math.isnan(eps) or math.isinf(eps):
        raise ValidationException("Softening parameter must be a finite number")


def validateTheta(theta):  # error_handling.cpp:115-123
    if theta < 0 or theta > 2.0:
        raise ValidationException("Barnes-Hut theta must be between 0 and 2")
    if math.isnan(theta) or math.isinf(theta):
        raise ValidationException("Barnes-Hut theta must be a finite number")


def validateSimulationConfig(cfg: SimulationConfig):
    validateParticleCountRange(cfg.particle_count)
    validateTimeStep(cfg.dt)
    validateSoftening(cfg.softening)
    if cfg.force_method == ForceMethod.BARNES_HUT:
        validateTheta(cfg.barnes_hut_theta)
    if cfg.G <= 0 or not _finite(cfg.G):
        raise ValidationException("Gravitational constant must be positive and finite")
    if cfg.force_method == ForceMethod.SPATIAL_HASH:
        if cfg.spatial_hash_cell_size <= 0 or not _finite(cfg.spatial_hash_cell_size):
            raise ValidationException("Spatial hash cell size must be positive and finite")
        if cfg.spatial_hash_cutoff <= 0 or not _finite(cfg.spatial_hash_cutoff):
            raise ValidationException("Spatial hash cutoff must be positive and finite")
    if cfg.cuda_block_size <= 0 or cfg.cuda_block_size > 1024:
        raise ValidationException("CUDA block size must be between 1 and 1024")


# ---- context -------------------------------------------------------------------------------

class Context:
    """One per (process, device).  Launches go to torch's current stream of that device so that
    torch.cuda events / synchronize() order against them."""

    def __init__(self, device: int | None = None):
        lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.DeviceException("no HIP device available (this library has no CPU fallback)")
        if device is None:
            device = torch.cuda.current_device()
        self.device = int(device)
        self.torch_device = torch.device("cuda", self.device)
        stream = torch.cuda.current_stream(self.torch_device).cuda_stream
        h = C.c_void_p()
        check(lib.nbody_hip_ctx_create(C.byref(h), self.device, C.c_void_p(stream)))
        self._h = h
        self._lib = lib
        _lib.track(self, "context")

    @property
    def handle(self):
        return self._h

    def use_stream(self, stream: "torch.cuda.Stream | None"):
        ptr = None if stream is None else C.c_void_p(stream.cuda_stream)
        check(self._lib.nbody_hip_ctx_set_stream(self._h, ptr))

    def synchronize(self):
        check(self._lib.nbody_hip_ctx_synchronize(self._h))

    def capture(self):
        """`with ctx.capture() as rec: ...calls...` records the calls into rec.graph (a StepGraph)
        instead of executing them (include/nbody_hip.h, "step graphs")."""
        return _Capture(self)

    def tuning(self, variant=-1, targets_per_lane=0, source_splits=0):
        """Experiment knobs of the Direct kernels (nbody_hip_direct_tuning); no arguments = automatic.  variant: 0 scalar
        body, 1 packed body, 2 scalar-cache sources, 3 symmetric kernel at any size, 4 the symmetric kernel with every
        fp64 I-side sum in LDS (16 bodies per lane: one workgroup per CU instead of two; bit for bit the result of 3)."""
        check(self._lib.nbody_hip_direct_tuning(self._h, variant, targets_per_lane, source_splits))

    def deterministic(self, mode=True):
        """Direct forces bitwise reproducible (nbody_hip_direct_deterministic): 0 / False = fp64 atomics, 1 / True =
        slot planes when they fit the budget (default), 2 = slot planes required (else ResourceException)."""
        check(self._lib.nbody_hip_direct_deterministic(self.handle, int(mode)))

    def slotBudget(self, nbytes: int = 0):
        """most bytes of slot planes the deterministic Direct form may take (0 = default, 24 GiB)"""
        check(self._lib.nbody_hip_direct_slot_budget(self.handle, nbytes))

    def directInfo(self, count: int = 0, eps2: float = 1.0) -> dict:
        """What a Direct all-pairs call at `count` bodies runs, and what the last call ran (nbody_hip_direct_info)."""
        from ._lib import DirectInfoStruct
        s = DirectInfoStruct()
        check(self._lib.nbody_hip_direct_info(self.handle, count, eps2, C.byref(s)))
        out = {k: getattr(s, k) for k, _ in DirectInfoStruct._fields_ if not k.startswith("reserved")}
        out["kernel_name"] = ("one-sided", "symmetric+atomics", "symmetric+slots")[s.kernel]
        return out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.nbody_hip_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            if not _lib.finalizing():  # (else: closed by the exit hook _lib.close_all, or the runtime is going down)
                self.close()
        except Exception:
            pass


class StepGraph:
    """A recorded sequence of launches (hipGraphExec); launch(k) replays it k times in order."""

    def __init__(self, ctx: Context, handle):
        self._ctx, self._h = ctx, handle
        _lib.track(self, "graph")

    def launch(self, times: int = 1):
        check(self._ctx._lib.nbody_hip_graph_launch(self._h, int(times)))

    def close(self):
        if self._h is not None and self._h.value and self._ctx._h.value:
            self._ctx._lib.nbody_hip_graph_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            if not _lib.finalizing():  # (else: closed by the exit hook _lib.close_all, or the runtime is going down)
                self.close()
        except Exception:
            pass


class _Capture:
    def __init__(self, ctx: Context):
        self.ctx, self.graph = ctx, None

    def __enter__(self):
        check(self.ctx._lib.nbody_hip_capture_begin(self.ctx.handle))
        return self

    def __exit__(self, et, ev, tb):
        h = C.c_void_p()
        rc = self.ctx._lib.nbody_hip_capture_end(self.ctx.handle, C.byref(h))  # always restores the context
        if et is None:
            check(rc)
            self.graph = StepGraph(self.ctx, h)
        elif rc == 0:
            self.ctx._lib.nbody_hip_graph_destroy(h)
        return False


_default_ctx: dict[int, Context] = {}


def default_context(device: int | None = None) -> Context:
    if device is None:
        device = torch.cuda.current_device() if torch.cuda.is_available() else 0
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


# ---- particle data ---------------------------------------------------------------------------

class ParticleData:
    """13 float32 arrays + count (types.hpp:234-276).  `where` is "device" (torch tensors on the
    GPU) or "host" (numpy arrays)."""

    def __init__(self):
        self.count = 0
        self.where = None
        for f in FIELDS:
            setattr(self, f, None)

    def struct(self) -> ParticleDataStruct:
        s = ParticleDataStruct()
        for f in FIELDS:
            a = getattr(self, f)
            if a is None:
                ptr = None
            elif isinstance(a, torch.Tensor):
                ptr = a.data_ptr()
            else:
                ptr = a.ctypes.data
            setattr(s, f, ptr)
        s.count = self.count
        return s


class ParticleDataManager:
    """particle_data.hpp:9-36 / particle_init.cu:143-283."""

    @staticmethod
    def allocateDevice(data: ParticleData, count: int, device=None):
        validateParticleCountRange(count)
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        # one slab, 64-float (256 B) aligned sub-arrays, zero-initialised (ref zeroes acc*)
        stride = (count + 63) // 64 * 64
        slab = torch.zeros(13 * stride, dtype=torch.float32, device=dev)
        for k, f in enumerate(FIELDS):
            setattr(data, f, slab[k * stride:k * stride + count])
        data._slab = slab
        data.count = count
        data.where = "device"

    @staticmethod
    def freeDevice(data: ParticleData):
        for f in FIELDS:
            setattr(data, f, None)
        data._slab = None
        data.count = 0

    @staticmethod
    def allocateHost(data: ParticleData, count: int):
        for f in FIELDS:
            setattr(data, f, np.zeros(count, dtype=np.float32))
        data.count = count
        data.where = "host"

    @staticmethod
    def freeHost(data: ParticleData):
        for f in FIELDS:
            setattr(data, f, None)
        data.count = 0

    _COPIED = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "acc_x", "acc_y", "acc_z",
               "mass")  # acc_old is not copied by the reference either (particle_init.cu:257-283)

    @staticmethod
    def copyToDevice(d_data: ParticleData, h_data: ParticleData):
        if h_data.count > d_data.count:
            raise ValidationException("host count exceeds device capacity")
        n = h_data.count
        for f in ParticleDataManager._COPIED:
            getattr(d_data, f)[:n].copy_(torch.from_numpy(np.ascontiguousarray(getattr(h_data, f)[:n])))

    @staticmethod
    def copyToHost(h_data: ParticleData, d_data: ParticleData):
        if d_data.count > h_data.count:
            raise ValidationException("device count exceeds host capacity")
        n = d_data.count
        for f in ParticleDataManager._COPIED:
            getattr(h_data, f)[:n] = getattr(d_data, f)[:n].cpu().numpy()


# ---- host initialisers ------------------------------------------------------------------------

@dataclass
class UniformDistParams:  # types.hpp:330-335
    min_bounds: tuple = (0.0, 0.0, 0.0)
    max_bounds: tuple = (0.0, 0.0, 0.0)
    min_mass: float = 1.0
    max_mass: float = 1.0


@dataclass
class SphericalDistParams:  # types.hpp:346-351
    center: tuple = (0.0, 0.0, 0.0)
    radius: float = 10.0
    min_mass: float = 1.0
    max_mass: float = 1.0


@dataclass
class DiskDistParams:  # types.hpp:362-369
    center: tuple = (0.0, 0.0, 0.0)
    radius: float = 10.0
    thickness: float = 1.0
    min_mass: float = 1.0
    max_mass: float = 1.0
    rotation_speed: float = 1.0


class _Mt19937Floats:
    """std::mt19937(seed) feeding std::uniform_real_distribution<float> the way libstdc++ does
    (bits/random.tcc generate_canonical<float,24>): one 32-bit draw x per variate,
    u = float(x) / 2^32 (x rounded to nearest-even float; u >= 1 -> nextafter(1,0)), result
    a + (b - a) * u in float32.  numpy's legacy RandomState(seed) is the same init_genrand stream."""

    def __init__(self, seed: int):
        self._bits = np.random.RandomState(seed)._bit_generator

    def canonical(self, count: int) -> np.ndarray:
        x = self._bits.random_raw(count).astype(np.uint32)
        u = x.astype(np.float32) / np.float32(4294967296.0)
        return np.minimum(u, np.nextafter(np.float32(1), np.float32(0)))


def _dist(u, a, b):
    a, b = np.float32(a), np.float32(b)
    return u * (b - a) + a


class ParticleInitializer:
    """particle_data.hpp:38-57 / particle_init.cu:286-376: the three host recipes, drawing from the
    generator in the reference's order (per body).  Bit-exact for the uniform box; the sphere and
    disk go through cbrt / sin / cos / acos / sqrt, where numpy and glibc may differ in the last ulp
    (tests/test_system_cpu.py compares with the C++ facade built on libstdc++)."""

    @staticmethod
    def zeroVelocities(h: ParticleData):
        for f in ("vel_x", "vel_y", "vel_z"):
            getattr(h, f)[:] = 0

    @staticmethod
    def zeroAccelerations(h: ParticleData):
        for f in ("acc_x", "acc_y", "acc_z", "acc_old_x", "acc_old_y", "acc_old_z"):
            getattr(h, f)[:] = 0

    @staticmethod
    def initUniform(h: ParticleData, p: UniformDistParams, seed: int = 42):
        n = h.count
        u = _Mt19937Floats(seed).canonical(4 * n).reshape(n, 4)  # per body: x, y, z, mass
        for k, f in enumerate(("pos_x", "pos_y", "pos_z")):
            getattr(h, f)[:] = _dist(u[:, k], p.min_bounds[k], p.max_bounds[k])
        h.mass[:] = _dist(u[:, 3], p.min_mass, p.max_mass)
        ParticleInitializer.zeroVelocities(h)
        ParticleInitializer.zeroAccelerations(h)

    @staticmethod
    def initSpherical(h: ParticleData, p: SphericalDistParams, seed: int = 42):
        n = h.count
        f32 = np.float32
        u = _Mt19937Floats(seed).canonical(4 * n).reshape(n, 4)  # radius, azimuth, polar, mass
        r = np.cbrt(_dist(u[:, 0], 0, 1)) * f32(p.radius)
        theta = _dist(u[:, 1], 0, 1) * f32(2.0) * f32(3.14159265)
        phi = np.arccos(f32(2.0) * _dist(u[:, 2], 0, 1) - f32(1.0))
        h.pos_x[:] = f32(p.center[0]) + r * np.sin(phi) * np.cos(theta)
        h.pos_y[:] = f32(p.center[1]) + r * np.sin(phi) * np.sin(theta)
        h.pos_z[:] = f32(p.center[2]) + r * np.cos(phi)
        h.mass[:] = _dist(u[:, 3], p.min_mass, p.max_mass)
        ParticleInitializer.zeroVelocities(h)
        ParticleInitializer.zeroAccelerations(h)

    @staticmethod
    def initDisk(h: ParticleData, p: DiskDistParams, seed: int = 42):
        n = h.count
        f32 = np.float32
        u = _Mt19937Floats(seed).canonical(4 * n).reshape(n, 4)  # radius, azimuth, height, mass
        r = np.sqrt(_dist(u[:, 0], 0, 1)) * f32(p.radius)
        theta = _dist(u[:, 1], 0, 1) * f32(2.0) * f32(3.14159265)
        z = (_dist(u[:, 2], 0, 1) - f32(0.5)) * f32(p.thickness)
        h.pos_x[:] = f32(p.center[0]) + r * np.cos(theta)
        h.pos_y[:] = f32(p.center[1]) + r * np.sin(theta)
        h.pos_z[:] = f32(p.center[2]) + z
        v = f32(p.rotation_speed) * np.sqrt(r)
        h.vel_x[:] = -v * np.sin(theta)
        h.vel_y[:] = v * np.cos(theta)
        h.vel_z[:] = 0
        h.mass[:] = _dist(u[:, 3], p.min_mass, p.max_mass)
        ParticleInitializer.zeroAccelerations(h)


# ---- force calculators -----------------------------------------------------------------------

def _phi_arg(phi, count: int):
    """The `phi` argument of the potential calls: None, or a contiguous float32 device tensor of `count` elements."""
    if phi is None:
        return None
    if not (isinstance(phi, torch.Tensor) and phi.dtype == torch.float32 and phi.device.type == "cuda"
            and phi.is_contiguous() and phi.dim() == 1 and phi.numel() == count):
        raise ValidationException(f"phi must be a contiguous float32 device tensor of {count} elements")
    return phi.data_ptr()


def _field_args(points, out):
    """The `points` / `out` arguments of the field calls: points = a float32 device tensor [M, 3] or [M, 4] (padded /
    made contiguous here), out = None or a contiguous float32 device tensor [M, 4].  Returns (points4, out)."""
    if not (isinstance(points, torch.Tensor) and points.dtype == torch.float32 and points.device.type == "cuda"
            and points.dim() == 2 and points.shape[1] in (3, 4)):
        raise ValidationException("points must be a float32 device tensor of shape [M, 3] or [M, 4]")
    m = points.shape[0]
    if points.shape[1] == 3:
        points = torch.nn.functional.pad(points, (0, 1))
    points = points.contiguous()
    if out is None:
        out = torch.empty((m, 4), dtype=torch.float32, device=points.device)
    elif not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.device == points.device
              and out.is_contiguous() and tuple(out.shape) == (m, 4)):
        raise ValidationException(f"out must be a contiguous float32 device tensor of shape [{m}, 4]")
    return points, out


class ForceCalculator:
    """force_calculator.hpp:36-89: caches eps, eps^2, G; computeForces overwrites acc_*."""

    def __init__(self, ctx: Context | None = None):
        self.softening_eps_ = 0.01
        self.softening_eps2_ = 0.0001
        self.G_ = 1.0
        self._ctx = ctx

    @property
    def ctx(self) -> Context:
        if self._ctx is None:
            self._ctx = default_context()
        return self._ctx

    def setSofteningParameter(self, eps):
        self.softening_eps_ = float(eps)
        # eps*eps in fp32, as the C++ setter does with float members
        self.softening_eps2_ = float(np.float32(eps) * np.float32(eps))

    def setGravitationalConstant(self, G):
        self.G_ = float(G)

    def getSofteningParameter(self):
        return self.softening_eps_

    def getGravitationalConstant(self):
        return self.G_

    def computeForces(self, d_particles: ParticleData):
        raise NotImplementedError

    def computePotential(self, d_particles: ParticleData, phi=None) -> float:
        """PE = 1/2 sum m_i phi_i of this method's own model, and phi_i into `phi` (a float32 device tensor of `count`
        elements) when given.  Here: the Direct sum (nbody_hip_direct_potential), for every calculator that does not
        override it; Barnes-Hut and the spatial hash build their structure and use its potential."""
        ptr = _phi_arg(phi, d_particles.count)
        s = d_particles.struct()
        pe = C.c_double()
        check(self.ctx._lib.nbody_hip_direct_potential(self.ctx.handle, C.byref(s), self.G_, self.softening_eps_,
                                                       ptr, C.byref(pe)))
        return pe.value

    def computeField(self, d_particles: ParticleData, points, out=None) -> torch.Tensor:
        """{ax, ay, az, phi} of this method's own model at `points` (float32 device tensor [M, 3] or [M, 4]) as an
        [M, 4] tensor (`out` when given).  Here: the Direct sum over the bodies (nbody_hip_direct_field), for every
        calculator that does not override it; Barnes-Hut and the spatial hash build their structure and use its field.
        Writes no acc_*."""
        p4, out = _field_args(points, out)
        s = d_particles.struct()
        check(self.ctx._lib.nbody_hip_direct_field(self.ctx.handle, C.byref(s), p4.data_ptr(), p4.shape[0], self.G_,
                                                   self.softening_eps_, out.data_ptr()))
        return out

    def _graph_key(self):
        """everything a recorded step bakes in besides the arrays"""
        return (self.G_, self.softening_eps_)

    def getMethod(self) -> ForceMethod:
        raise NotImplementedError


class DirectForceCalculator(ForceCalculator):
    """force_calculator.hpp:101-121 / force_direct.cu:101-106."""

    def __init__(self, block_size: int = 256, ctx: Context | None = None):
        super().__init__(ctx)
        self.block_size_ = block_size

    def computeForces(self, d_particles: ParticleData):
        s = d_particles.struct()
        check(self.ctx._lib.nbody_hip_direct_forces(self.ctx.handle, C.byref(s), self.G_,
                                                    self.softening_eps2_, self.block_size_))

    def getMethod(self):
        return ForceMethod.DIRECT_N2

    def setBlockSize(self, size):
        self.block_size_ = size

    def getBlockSize(self):
        return self.block_size_


class GroupCatalogue:
    """The friends-of-friends groups of one SpatialHashGrid.findGroups call (include/nbody_hip_groups.h), on the device:
    labels [N] int32, the lowest body index of every body's group; the groups of at least min_members bodies ascending by
    label, group g = members[offsets[g] : offsets[g + 1]] (int32), members ascending by body index."""

    def __init__(self, labels: torch.Tensor, offsets: torch.Tensor, members: torch.Tensor, linking_length: float,
                 min_members: int):
        self.labels, self.offsets, self.members = labels, offsets, members
        self.n_groups = int(offsets.numel()) - 1
        self.n_members = int(members.numel())
        self.linking_length, self.min_members = float(linking_length), int(min_members)

    def sizes(self) -> torch.Tensor:
        """bodies per group, [n_groups] int32 on the device"""
        return self.offsets[1:] - self.offsets[:-1]

    def systems(self, d_particles: ParticleData):
        """-> (ParticleData of the members gathered in catalogue order, offsets as an int64 device tensor): the layout
        systems_diagnostics and ic.concat use, so per-group fp64 mass, centre of mass, momenta and energies come from
        that call (groups of at most 4,096 members).  Plain torch indexing: plumbing, not a kernel."""
        if self.n_members == 0:
            raise ValidationException("the catalogue holds no group: nothing to gather")
        if d_particles.count != self.labels.numel():
            raise ValidationException(f"the catalogue was found on {self.labels.numel()} bodies, the particle data holds "
                                      f"{d_particles.count}")
        out = ParticleData()
        ParticleDataManager.allocateDevice(out, self.n_members, self.members.device.index)
        take = self.members.to(torch.int64)
        for f in FIELDS:
            getattr(out, f).copy_(getattr(d_particles, f)[take])
        return out, self.offsets.to(torch.int64).contiguous()

    def properties(self, d_particles: ParticleData, phi=None, ctx: "Context | None" = None) -> np.ndarray:
        """fp64 properties of every group, whatever its size (nbody_hip_groups_properties): a numpy structured array
        (GROUP_PROPS_DTYPE), one row per group -- mass, com, vel, ang_mom, kinetic, inertia, r_max, potential, phi_min,
        n, label, r_max_body, phi_min_body, status.  phi: the per-body potential of any force method (a float32 device
        tensor of d_particles.count entries, original body order) or None.  Blocks for the copy."""
        return groups_properties(ctx or default_context(self.offsets.device.index), d_particles, self.offsets,
                                 self.members, phi)

    def properties_into(self, d_particles: ParticleData, out: torch.Tensor, phi=None, ctx: "Context | None" = None):
        """The same, asynchronous, into `out` (group_props_tensor): reads nothing back, and can be recorded into a step
        graph once a call of these sizes has run eagerly.  Returns `out`."""
        return groups_properties_into(ctx or default_context(self.offsets.device.index), d_particles, self.offsets,
                                      self.members, out, phi)

    def radialProfile(self, d_particles: ParticleData, centres, cuts, mode="mass", vels=None, sorted_members=None,
                      sorted_q=None, ctx: "Context | None" = None):
        """Radial profiles of every group about `centres` (groups_radial_profile; include/nbody_hip_radial.h):
        -> (groups [n_groups] RADIAL_GROUP_DTYPE, shells [n_groups, n_cuts] RADIAL_SHELL_DTYPE).  Blocks for the copy."""
        return groups_radial_profile(ctx or default_context(self.offsets.device.index), d_particles, self.offsets,
                                     self.members, centres, cuts, mode, vels, sorted_members, sorted_q)

    def lagrangianRadii(self, d_particles: ParticleData, centres, fractions, ctx: "Context | None" = None) -> np.ndarray:
        """The radii that enclose the mass fractions `fractions` of every group about `centres`: [n_groups, n_fractions]
        float64 (the `radius` column of radialProfile in mass mode; 0 in the rows of a group with a non-zero status)."""
        return self.radialProfile(d_particles, centres, fractions, "mass", ctx=ctx)[1]["radius"].copy()


class NeighbourLists:
    """What SpatialHashGrid.neighbours returns (include/nbody_hip_neighbours.h), on the device, rows in ORIGINAL body
    order: index [N, k] int32 and dist2 [N, k] float32 ascending by (d2, index), -1 / +inf in unused slots (None without
    lists); rho [N] float64, the Casertano-Hut density (None without density); status [N] int32: 0 exact, 1
    window-limited, 2 fewer than k candidates, 3 the k-th neighbour coincident.  ParticleSystem.localDensity adds level
    [N] int32, the grid level that computed each body last, levels, their number, and cells, the cell size of each."""

    def __init__(self, k: int, index, dist2, rho, status, level=None):
        self.k, self.index, self.dist2, self.rho, self.status, self.level = int(k), index, dist2, rho, status, level
        self.levels, self.cells = None, None


NEIGHBOURS_MAX_K = 32
HOP_MAX_K = 32
HOP_STAGES = ("hop", "peaks", "records", "sort and fold", "unite and attach", "catalogue")


class HopCatalogue(GroupCatalogue):
    """The density-peak (HOP) groups of one hop_groups call (include/nbody_hip_hop.h), on the device: a GroupCatalogue
    (labels [N], offsets, members: properties, radialProfile, lagrangianRadii and systems work on it unchanged) whose
    label is root[peak], -1 for a body in no group; plus peak [N] int32, the density maximum every body's chain ends at;
    group_peak [n_groups] int32, the densest peak of every group; n_peaks; rounds, the attachment rounds evaluated;
    status (1: a neighbour index at or past N, nothing was grouped); and the parameters.  neighbours: the
    NeighbourLists the groups were found on, when the call computed them (hopGroups)."""

    def __init__(self, labels, offsets, members, peak, group_peak, n_peaks: int, rounds: int, status: int, k: int, n_hop: int,
                 n_merge: int, delta_outer: float, delta_saddle: float, delta_peak: float, min_members: int):
        super().__init__(labels, offsets, members, float("nan"), min_members)
        self.peak, self.group_peak = peak, group_peak
        self.n_peaks, self.rounds, self.status = int(n_peaks), int(rounds), int(status)
        self.k, self.n_hop, self.n_merge = int(k), int(n_hop), int(n_merge)
        self.delta_outer, self.delta_saddle, self.delta_peak = float(delta_outer), float(delta_saddle), float(delta_peak)
        self.neighbours = None
        self.stage_ms = None  # device milliseconds of the six stages (HOP_STAGES) of the search, None with status 1


def hop_groups(ctx: Context, index: torch.Tensor, rho: torch.Tensor, n_hop: int, n_merge: int, delta_outer: float,
               delta_saddle=None, delta_peak=None, min_members: int = 1) -> HopCatalogue:
    """Density-peak groups from neighbour lists and densities (nbody_hip_hop_groups): index [N, k] int32 and rho [N]
    float64 contiguous device tensors -- the index and rho of a NeighbourLists, or any lists; every body hops to the
    densest of its first n_hop neighbours, the basins of the density maxima are regrouped by the saddle densities found
    over the first n_merge neighbours.  delta_saddle, delta_peak: HOP's defaults 2.5 and 3 times delta_outer.  Blocks
    (record count, one word per attachment round, counts); bitwise reproducible."""
    for name, t, dt, dim in (("index", index, torch.int32, 2), ("rho", rho, torch.float64, 1)):
        if not (isinstance(t, torch.Tensor) and t.dtype == dt and t.dim() == dim and t.is_contiguous() and t.device.type == "cuda"):
            raise ValidationException(f"{name} must be a contiguous {dim}-dimensional {dt} device tensor")
    if index.device != rho.device or index.device != ctx.torch_device:
        raise ValidationException("index and rho must live on the device of the context")
    n, k = int(index.shape[0]), int(index.shape[1])
    if rho.numel() != n:
        raise ValidationException(f"index has {n} rows, rho {rho.numel()} entries")
    for name, v in (("n_hop", n_hop), ("n_merge", n_merge), ("min_members", min_members)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool):
            raise ValidationException(f"{name} must be an integer")
    if n == 0:
        raise ValidationException("Particle count must be greater than 0")
    if n > 2 ** 30:
        raise ValidationException("body count exceeds 2^30")
    d_outer = float(delta_outer)
    d_saddle = 2.5 * d_outer if delta_saddle is None else float(delta_saddle)
    d_peak = 3.0 * d_outer if delta_peak is None else float(delta_peak)
    params = _lib.HopParamsStruct(int(n_hop), int(n_merge), int(min_members), 0, d_outer, d_saddle, d_peak)
    dev = index.device
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    peak = torch.empty(n, dtype=torch.int32, device=dev)
    counts = (C.c_longlong * 5)()
    lib = ctx._lib
    check(lib.nbody_hip_hop_groups(ctx.handle, n, k, index.data_ptr() if n else None, rho.data_ptr() if n else None,
                                   C.byref(params), labels.data_ptr() if n else None, peak.data_ptr() if n else None,
                                   C.byref(counts)))
    offsets = torch.empty(counts[0] + 1, dtype=torch.int32, device=dev)
    members = torch.empty(counts[1], dtype=torch.int32, device=dev)
    group_peak = torch.empty(counts[0], dtype=torch.int32, device=dev)
    check(lib.nbody_hip_hop_groups_copy(ctx.handle, offsets.data_ptr(), members.data_ptr() if counts[1] else None,
                                        group_peak.data_ptr() if counts[0] else None))
    cat = HopCatalogue(labels, offsets, members, peak, group_peak, counts[2], counts[3], counts[4], k, n_hop, n_merge,
                       d_outer, d_saddle, d_peak, min_members)
    if cat.status == 0:
        ms = (C.c_float * 6)()
        check(lib.nbody_hip_hop_stage_times(ctx.handle, C.byref(ms)))
        cat.stage_ms = dict(zip(HOP_STAGES, (float(v) for v in ms)))
    return cat


def _hop_on_lists(ctx: Context, res: "NeighbourLists", n_hop, n_merge, delta_outer, delta_saddle, delta_peak,
                  min_members) -> HopCatalogue:
    """hop_groups on the lists and densities of a neighbour search; delta_outer None: the lower median of the densities"""
    if delta_outer is None:
        delta_outer = float(torch.nanmedian(res.rho)) if res.rho.numel() else 0.0
    cat = hop_groups(ctx, res.index, res.rho, res.k if n_hop is None else n_hop, n_merge, delta_outer, delta_saddle, delta_peak,
                     min_members)
    cat.neighbours = res
    return cat


class SpatialHashGrid:
    """spatial_hash_grid.hpp:9-59 / force_spatial_hash.cu:155-361."""

    def __init__(self, max_particles: int, cell_size: float = 1.0, ctx: Context | None = None):
        self.ctx = ctx or default_context()
        self.max_particles_ = int(max_particles)
        self.cell_size_ = float(cell_size)
        h = C.c_void_p()
        check(self.ctx._lib.nbody_hip_grid_create(self.ctx.handle, self.max_particles_,
                                                  self.cell_size_, C.byref(h)))
        self._h = h
        _lib.track(self, "grid")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            if self.ctx.handle.value:  # (a closed context has taken its stream with it: nothing left to wait for)
                self.ctx._lib.nbody_hip_grid_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            if not _lib.finalizing():  # (else: closed by the exit hook _lib.close_all, or the runtime is going down)
                self.close()
        except Exception:
            pass

    def setCellSize(self, size):
        check(self.ctx._lib.nbody_hip_grid_set_cell_size(self._h, size))
        self.cell_size_ = float(size)

    def tuning(self, kernel: int = 0):
        """force kernel: 0 automatic, 1 cell-run, 2 / 3 / 4 wave-per-cell with 1 / 2 / 4 bodies per lane, 6 = 3 with the
        window filtered by the box of the cell's bodies (crowded cells), 5 = timing probe (not forces), 7 = two-phase form,
        8 = one lane per body, 9 = split form (8 for the light cells, 3 for the crowded ones), 10 = two bodies of one cell
        per lane"""
        check(self.ctx._lib.nbody_hip_grid_tuning(self._h, kernel))

    def build(self, d_particles: ParticleData):
        s = d_particles.struct()
        self._last_count = d_particles.count
        check(self.ctx._lib.nbody_hip_grid_build(self._h, C.byref(s)))

    def driftBuild(self, d_particles: ParticleData, dt: float):
        """The drift of a Velocity-Verlet step and this build in one pass (nbody_hip_grid_drift_build)."""
        s = d_particles.struct()
        self._last_count = d_particles.count
        check(self.ctx._lib.nbody_hip_grid_drift_build(self._h, C.byref(s), dt))

    def computeForces(self, d_particles: ParticleData, cutoff: float, G: float, eps: float):
        s = d_particles.struct()
        check(self.ctx._lib.nbody_hip_grid_compute_forces(self._h, C.byref(s), cutoff, G, eps))

    def computePotential(self, d_particles: ParticleData, cutoff: float, G: float, eps: float, phi=None) -> float:
        """The shifted truncated potential over the force's pair set on the grid as built (nbody_hip_grid_potential):
        returns PE = 1/2 sum m phi, writes phi into `phi` when given."""
        ptr = _phi_arg(phi, d_particles.count)
        s = d_particles.struct()
        pe = C.c_double()
        check(self.ctx._lib.nbody_hip_grid_potential(self._h, C.byref(s), cutoff, G, eps, ptr, C.byref(pe)))
        return pe.value

    def computeField(self, points, cutoff: float, G: float, eps: float, out=None) -> torch.Tensor:
        """{ax, ay, az, phi} of the grid as built at `points` (nbody_hip_grid_field): the truncated force and the shifted
        truncated potential over the 27-cell window of each point's cell.  [M, 4]; fills `out` when given."""
        p4, out = _field_args(points, out)
        check(self.ctx._lib.nbody_hip_grid_field(self._h, p4.data_ptr(), p4.shape[0], cutoff, G, eps, out.data_ptr()))
        return out

    def findGroups(self, linking_length: float, min_members: int = 1) -> GroupCatalogue:
        """Friends-of-friends groups of the grid as built (nbody_hip_grid_groups): bodies of neighbouring cells closer
        than linking_length (fp32 d2 < fl(b * b), coincident bodies included) are linked; linking_length may not exceed
        the cell size of the build.  Blocks for the two counts."""
        lib = self.ctx._lib
        built = C.c_size_t()
        check(lib.nbody_hip_grid_count(self._h, C.byref(built)))
        dev = self.ctx.torch_device
        labels = torch.empty(built.value, dtype=torch.int32, device=dev)
        counts = (C.c_longlong * 2)()
        check(lib.nbody_hip_grid_groups(self._h, linking_length, min_members, labels.data_ptr() if built.value else None,
                                        C.byref(counts)))
        self._group_count = int(counts[0])
        offsets = torch.empty(counts[0] + 1, dtype=torch.int32, device=dev)
        members = torch.empty(counts[1], dtype=torch.int32, device=dev)
        check(lib.nbody_hip_grid_groups_copy(self._h, offsets.data_ptr(), members.data_ptr() if counts[1] else None))
        return GroupCatalogue(labels, offsets, members, linking_length, min_members)

    def groupProperties(self, d_particles: ParticleData, phi=None) -> np.ndarray:
        """The properties (GroupCatalogue.properties) of the catalogue this grid holds since its last findGroups, read
        from the grid's own arrays (nbody_hip_grid_groups_properties).  Blocks for the copy."""
        n_groups = getattr(self, "_group_count", None)  # (of the last findGroups on this handle: the size of `out`)
        if n_groups is None:
            raise StateException("no group catalogue: call findGroups after the last build first")
        out = group_props_tensor(n_groups, self.ctx.torch_device)
        ptr = _phi_arg(phi, d_particles.count)
        s = d_particles.struct()
        check(self.ctx._lib.nbody_hip_grid_groups_properties(self._h, C.byref(s), ptr,
                                                             out.data_ptr() if n_groups else None))
        self.ctx.synchronize()
        return group_props_array(out)

    def groupRadialProfile(self, d_particles: ParticleData, centres, cuts, mode="mass", vels=None, sorted_members=None,
                           sorted_q=None):
        """The radial profiles (GroupCatalogue.radialProfile) of the catalogue this grid holds since its last findGroups,
        read from the grid's own arrays (nbody_hip_grid_groups_radial_profile).  Blocks for the copy."""
        n_groups = getattr(self, "_group_count", None)
        if n_groups is None:
            raise StateException("no group catalogue: call findGroups after the last build first")
        dev = self.ctx.torch_device
        cuts_arr, mode_id = _radial_cuts(cuts, mode)
        cen, vel = _radial_centres("centres", centres, n_groups, dev), _radial_centres("vels", vels, n_groups, dev)
        groups, shells = radial_tensors(n_groups, cuts_arr.size, dev)
        for name, t, dt in (("sorted_members", sorted_members, torch.int32), ("sorted_q", sorted_q, torch.float32)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == dt and t.is_contiguous() and t.device == cen.device):
                raise ValidationException(f"{name} must be a contiguous {dt} device tensor of n_members elements")
        s = d_particles.struct()
        check(self.ctx._lib.nbody_hip_grid_groups_radial_profile(
            self._h, C.byref(s), cen.data_ptr() if n_groups else None, None if vel is None else vel.data_ptr(),
            cuts_arr.ctypes.data, cuts_arr.size, mode_id, groups.data_ptr() if n_groups else None,
            shells.data_ptr() if n_groups else None, None if sorted_members is None else sorted_members.data_ptr(),
            None if sorted_q is None else sorted_q.data_ptr()))
        self.ctx.synchronize()
        return radial_arrays(groups, shells, cuts_arr.size)

    def neighbours(self, k: int, lists: bool = True, density: bool = False, status=None, out=None) -> NeighbourLists:
        """The k nearest candidates (1 <= k <= 32) of every body on the grid as built (nbody_hip_grid_neighbours): the
        bodies of the 27-cell window, ordered by (fp32 d2, body index).  Asynchronous; bitwise reproducible.
        status: the status tensor of an earlier call on a FINER build of the same bodies -- the call then refines in
        place: bodies whose status is 0 are skipped (none of their outputs is written), every other body is recomputed
        on this build.  out: the NeighbourLists of that earlier call, whose tensors are written in place (its status is
        the default of `status`); without it the skipped rows of fresh tensors hold -1 / +inf / 0."""
        lib = self.ctx._lib
        built = C.c_size_t()
        check(lib.nbody_hip_grid_count(self._h, C.byref(built)))
        n, dev = built.value, self.ctx.torch_device
        if not isinstance(k, (int, np.integer)) or isinstance(k, bool):
            raise ValidationException("k must be an integer")
        k = int(k)
        kk = min(max(k, 1), NEIGHBOURS_MAX_K)  # (the library refuses a k out of range: the tensors only need a size)
        if out is not None:
            if not isinstance(out, NeighbourLists) or out.k != k or out.status is None or out.status.numel() != n:
                raise ValidationException("out must be the NeighbourLists of an earlier call with this k on these bodies")
            if status is None:
                status = out.status
        refine = status is not None
        if refine and not (isinstance(status, torch.Tensor) and status.dtype == torch.int32 and status.device.type == "cuda"
                           and status.is_contiguous() and status.dim() == 1 and status.numel() == n):
            raise ValidationException(f"status must be a contiguous int32 device tensor of {n} elements")
        if not refine:
            status = torch.empty(n, dtype=torch.int32, device=dev)
        index = dist2 = rho = None
        if lists:
            if out is not None and out.index is not None:
                index, dist2 = out.index, out.dist2
            elif refine:
                index = torch.full((n, kk), -1, dtype=torch.int32, device=dev)
                dist2 = torch.full((n, kk), float("inf"), dtype=torch.float32, device=dev)
            else:
                index = torch.empty((n, kk), dtype=torch.int32, device=dev)
                dist2 = torch.empty((n, kk), dtype=torch.float32, device=dev)
        if density:
            if out is not None and out.rho is not None:
                rho = out.rho
            else:
                rho = (torch.zeros if refine else torch.empty)(n, dtype=torch.float64, device=dev)

        def ptr(t):
            return t.data_ptr() if t is not None and n else None

        check(lib.nbody_hip_grid_neighbours(self._h, k, 1 if refine else 0, ptr(index), ptr(dist2), ptr(rho),
                                            status.data_ptr() if n else None))
        if out is not None:
            out.index, out.dist2, out.rho, out.status = index, dist2, rho, status
            return out
        return NeighbourLists(k, index, dist2, rho, status)

    def localDensity(self, k: int = 6) -> NeighbourLists:
        """The Casertano-Hut density of every body from its k nearest candidates on the grid as built, without lists:
        rho [N] float64 and status [N] int32 of a NeighbourLists (status 1: computed from what the window holds)."""
        return self.neighbours(k, lists=False, density=True)

    def hopGroups(self, k: int = 16, n_hop=None, n_merge: int = 4, delta_outer=None, delta_saddle=None, delta_peak=None,
                  min_members: int = 1) -> HopCatalogue:
        """Density-peak (HOP) groups of the grid as built: neighbours(k) with lists and density, then hop_groups on them
        (n_hop None: k; delta_outer None: the lower median of the densities; delta_saddle / delta_peak None: 2.5 and 3 times
        delta_outer).  The lists are those of the 27-cell windows: a window-limited body hops among what its window
        holds (ParticleSystem.hopGroups resolves every body first).  The catalogue's `neighbours` holds the lists."""
        res = self.neighbours(k, lists=True, density=True)
        return _hop_on_lists(self.ctx, res, n_hop, n_merge, delta_outer, delta_saddle, delta_peak, min_members)

    def isWholeWindow(self) -> bool:
        """At most 2 cells along every axis: every body is in every window, and no status is window-limited."""
        return max(self.getGridDims()) <= 2

    def _info(self):
        dims, total = (C.c_int * 3)(), C.c_int()
        lo, hi = (C.c_float * 3)(), (C.c_float * 3)()
        check(self.ctx._lib.nbody_hip_grid_info(self._h, C.byref(dims), C.byref(total),
                                                C.byref(lo), C.byref(hi)))
        return list(dims), total.value, list(lo), list(hi)

    def getGridDims(self):
        return tuple(self._info()[0])

    def getCellSize(self):
        return self.cell_size_

    def getTotalCells(self):
        return self._info()[1]

    def getBoundingBox(self):
        _, _, lo, hi = self._info()
        return lo, hi

    def copyCellDataToHost(self):
        """-> (cell_start, cell_end, particle_cells, sorted_indices) as numpy int32 arrays."""
        dims, total, _, _ = self._info()
        n = self._count()
        cs, ce = np.empty(total, np.int32), np.empty(total, np.int32)
        pc, si = np.empty(n, np.int32), np.empty(n, np.int32)
        check(self.ctx._lib.nbody_hip_grid_copy_cell_data(self._h, cs.ctypes.data, ce.ctypes.data,
                                                          pc.ctypes.data, si.ctypes.data))
        return cs, ce, pc, si

    def _count(self):
        return self._last_count

    def copyCellStartArray(self):
        """The per-cell start array the force kernels read (nbody_hip_grid_copy_cell_lb): None when the last build made
        none, else (lb_base, lb_count, lb) with lb[c - lb_base] = bodies whose cell id is below c, lb_count + 1 int32."""
        has, base, count = C.c_int(), C.c_int(), C.c_int()
        lib = self.ctx._lib
        check(lib.nbody_hip_grid_copy_cell_lb(self._h, C.byref(has), C.byref(base), C.byref(count), None))
        if not has.value:
            return None
        lb = np.empty(count.value + 1, np.int32)
        check(lib.nbody_hip_grid_copy_cell_lb(self._h, None, None, None, lb.ctypes.data))
        return base.value, count.value, lb

    def unitList(self, cell_first: int, cell_end: int, chunk: int, min_cnt: int = 1, mode: int = 0):
        """The work list of the cells [cell_first, cell_end) as a force call makes it (nbody_hip_grid_unit_list; mode 0
        units, 1 with the light cells' bodies, 2 with their pairs) -> (units [capacity, 2], light [counts[3]], counts [4],
        capacity) as numpy int32 arrays."""
        lib = self.ctx._lib
        cap, counts = C.c_int(), (C.c_int * 4)()
        check(lib.nbody_hip_grid_unit_list(self._h, cell_first, cell_end, chunk, min_cnt, mode, None, None, None,
                                           C.byref(cap)))
        units = np.empty((cap.value, 2), np.int32)
        light = np.empty(self.max_particles_, np.int32)
        check(lib.nbody_hip_grid_unit_list(self._h, cell_first, cell_end, chunk, min_cnt, mode, units.ctypes.data,
                                           light.ctypes.data, C.byref(counts), C.byref(cap)))
        assert cap.value == units.shape[0]
        counts = np.array(list(counts), np.int32)
        return units, light[: max(0, min(int(counts[3]), light.size)) if mode else 0].copy(), counts, cap.value

    @staticmethod
    def getCellIndex(x, y, z, cell_size):
        """force_spatial_hash.cu:14-17: floor of each coordinate over the cell size (fp32)."""
        f = np.float32
        return tuple(int(np.floor(f(v) / f(cell_size))) for v in (x, y, z))

    def verifyCellAssignment(self, h_particles: ParticleData) -> bool:
        """force_spatial_hash.cu:333-362: every body lies inside the bounds of its (clamped) cell."""
        dims, _, lo, _ = self._info()
        _, _, pc, _ = self.copyCellDataToHost()
        cs = np.float32(self.cell_size_)
        cell = np.stack([pc % dims[0], (pc // dims[0]) % dims[1], pc // (dims[0] * dims[1])], 1)
        for a, f in enumerate(("pos_x", "pos_y", "pos_z")):
            p = getattr(h_particles, f)[: pc.size]
            exp = np.clip(np.floor((p - np.float32(lo[a])) / cs).astype(np.int64), 0, dims[a] - 1)
            if not np.array_equal(exp, cell[:, a]):
                return False
            cmin = np.float32(lo[a]) + cell[:, a].astype(np.float32) * cs
            if np.any(p < cmin) or np.any(p > cmin + cs):
                return False
        return True


class SpatialHashCalculator(ForceCalculator):
    """force_calculator.hpp:176-211 / force_spatial_hash.cu:364-377: the grid is created lazily at
    the first computeForces and sized from that particle count."""

    def __init__(self, cell_size: float = 1.0, cutoff_radius: float = 2.0, ctx: Context | None = None):
        super().__init__(ctx)
        self.grid_ = None
        self.cell_size_ = float(cell_size)
        self.cutoff_radius_ = float(cutoff_radius)

    def computeForces(self, d_particles: ParticleData):
        if self.grid_ is None:
            self.grid_ = SpatialHashGrid(d_particles.count, self.cell_size_, self.ctx)
        self.grid_._last_count = d_particles.count
        self.grid_.build(d_particles)
        self.grid_.computeForces(d_particles, self.cutoff_radius_, self.G_, self.softening_eps_)

    def computePotential(self, d_particles: ParticleData, phi=None) -> float:
        _phi_arg(phi, d_particles.count)
        if self.grid_ is None:
            self.grid_ = SpatialHashGrid(d_particles.count, self.cell_size_, self.ctx)
        self.grid_._last_count = d_particles.count
        self.grid_.build(d_particles)
        return self.grid_.computePotential(d_particles, self.cutoff_radius_, self.G_, self.softening_eps_, phi)

    def computeField(self, d_particles: ParticleData, points, out=None) -> torch.Tensor:
        p4, out = _field_args(points, out)
        if self.grid_ is None:
            self.grid_ = SpatialHashGrid(d_particles.count, self.cell_size_, self.ctx)
        self.grid_._last_count = d_particles.count
        self.grid_.build(d_particles)
        return self.grid_.computeField(p4, self.cutoff_radius_, self.G_, self.softening_eps_, out)

    def findGroups(self, d_particles: ParticleData, linking_length: float, min_members: int = 1) -> GroupCatalogue:
        """Builds this calculator's grid on d_particles and finds the friends-of-friends groups on it
        (SpatialHashGrid.findGroups).  linking_length may not exceed the grid's cell size."""
        if self.grid_ is None:
            self.grid_ = SpatialHashGrid(d_particles.count, self.cell_size_, self.ctx)
        self.grid_._last_count = d_particles.count
        self.grid_.build(d_particles)
        try:
            return self.grid_.findGroups(linking_length, min_members)
        except ValidationException as e:
            if "exceeds the cell size" in str(e):
                raise ValidationException(f"{e}; call setCellSize({linking_length:g}) or larger first (a calculator "
                                          "whose grid already exists keeps its cell: create a new one)") from None
            raise

    def neighbours(self, d_particles: ParticleData, k: int, lists: bool = True, density: bool = False) -> NeighbourLists:
        """Builds this calculator's grid on d_particles and finds the k nearest candidates of every body on it
        (SpatialHashGrid.neighbours)."""
        if self.grid_ is None:
            self.grid_ = SpatialHashGrid(d_particles.count, self.cell_size_, self.ctx)
        self.grid_._last_count = d_particles.count
        self.grid_.build(d_particles)
        return self.grid_.neighbours(k, lists, density)

    def hopGroups(self, d_particles: ParticleData, k: int = 16, n_hop=None, n_merge: int = 4, delta_outer=None,
                  delta_saddle=None, delta_peak=None, min_members: int = 1) -> HopCatalogue:
        """Builds this calculator's grid on d_particles and finds the density-peak groups on it
        (SpatialHashGrid.hopGroups)."""
        if self.grid_ is None:
            self.grid_ = SpatialHashGrid(d_particles.count, self.cell_size_, self.ctx)
        self.grid_._last_count = d_particles.count
        self.grid_.build(d_particles)
        return self.grid_.hopGroups(k, n_hop, n_merge, delta_outer, delta_saddle, delta_peak, min_members)

    def getMethod(self):
        return ForceMethod.SPATIAL_HASH

    def setCellSize(self, size):
        # force_calculator.hpp:199: a plain store.  A grid that already exists was constructed with
        # the earlier size and keeps it (the reference never re-creates or re-sizes its grid,
        # force_spatial_hash.cu:372-374); the new value is used by the next grid this calculator creates.
        self.cell_size_ = float(size)

    def setCutoffRadius(self, radius):
        self.cutoff_radius_ = float(radius)

    def getCellSize(self):
        return self.cell_size_

    def getCutoffRadius(self):
        return self.cutoff_radius_

    def getGrid(self):
        return self.grid_


# include/nbody/barnes_hut_tree.hpp:9-30 -- 76 bytes
OCTREE_NODE_DTYPE = np.dtype([("center", np.float32, 3), ("half_size", np.float32),
                              ("center_of_mass", np.float32, 3), ("total_mass", np.float32),
                              ("children", np.int32, 8), ("particle_index", np.int32),
                              ("is_leaf", np.bool_), ("_pad", np.uint8, 3),
                              ("particle_count", np.int32)])
assert OCTREE_NODE_DTYPE.itemsize == 76


class BarnesHutTree:
    """barnes_hut_tree.hpp:33-81 / force_barnes_hut.cu:204-519."""

    def __init__(self, max_particles: int, ctx: Context | None = None):
        self.ctx = ctx or default_context()
        self.max_particles_ = int(max_particles)
        h = C.c_void_p()
        check(self.ctx._lib.nbody_hip_tree_create(self.ctx.handle, self.max_particles_, C.byref(h)))
        self._h = h
        self._count = 0
        self.h_nodes_ = None
        _lib.track(self, "tree")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            if self.ctx.handle.value:
                self.ctx._lib.nbody_hip_tree_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            if not _lib.finalizing():  # (else: closed by the exit hook _lib.close_all, or the runtime is going down)
                self.close()
        except Exception:
            pass

    def setParams(self, max_depth: int = 20, leaf_max: int = 1):
        check(self.ctx._lib.nbody_hip_tree_set_params(self._h, max_depth, leaf_max))
        self._params = (int(max_depth), int(leaf_max))

    def tuning(self, replicas: int = 0, split_level: int = 0):
        check(self.ctx._lib.nbody_hip_tree_tuning(self._h, replicas, split_level))

    def limitNodes(self, max_nodes: int = 0):
        """cap the node arrays (nbody_hip_tree_limit_nodes): a tree that needs more is cut, forces stay correct"""
        check(self.ctx._lib.nbody_hip_tree_limit_nodes(self._h, max_nodes))

    def walkForm(self, form: int = 0):
        """walk without replicas: 0 automatic, 1 plain, 2 pair walk (cost-ordered), 3 pair walk in plain order"""
        check(self.ctx._lib.nbody_hip_tree_walk_form(self._h, form))

    def countVisits(self, enable: bool = True):
        """stats()["nodes_visited"] is only maintained when enabled (it costs a launch per walk)."""
        check(self.ctx._lib.nbody_hip_tree_count_visits(self._h, 1 if enable else 0))

    def setMultipoleOrder(self, order: int):
        """1 (default: monopoles) or 2 (monopoles + quadrupoles, nbody_hip_tree_set_multipole_order).  Takes effect at
        the next build; a walk or potential call before that rebuild raises StateException."""
        check(self.ctx._lib.nbody_hip_tree_set_multipole_order(self._h, int(order)))
        self._order = int(order)

    def getMultipoleOrder(self) -> int:
        o = C.c_int()
        check(self.ctx._lib.nbody_hip_tree_get_multipole_order(self._h, C.byref(o)))
        return o.value

    def copyMomentsToHost(self) -> np.ndarray:
        """(nodes, 6) float32 second moments (Sxx, Syy, Szz, Sxy, Sxz, Syz) about each node's centre of mass, in the
        node numbering of copyNodesToHost; StateException unless the tree was built at order 2."""
        n = self.getNodeCount()
        out = np.zeros((n, 6), np.float32)
        check(self.ctx._lib.nbody_hip_tree_copy_moments(self._h, out.ctypes.data, n))
        return out

    def build(self, d_particles: ParticleData):
        s = d_particles.struct()
        check(self.ctx._lib.nbody_hip_tree_build(self._h, C.byref(s)))
        self._count = d_particles.count

    def driftBuild(self, d_particles: ParticleData, dt: float):
        """The drift of a Velocity-Verlet step and this build in one pass (nbody_hip_tree_drift_build)."""
        s = d_particles.struct()
        check(self.ctx._lib.nbody_hip_tree_drift_build(self._h, C.byref(s), dt))
        self._count = d_particles.count

    def computeForces(self, d_particles: ParticleData, theta: float, G: float, eps: float):
        s = d_particles.struct()
        check(self.ctx._lib.nbody_hip_tree_compute_forces(self._h, C.byref(s), theta, G, eps))

    def computePotential(self, d_particles: ParticleData, theta: float, G: float, eps: float, phi=None) -> float:
        """The potential over the force walk's interaction list on the tree as built (nbody_hip_tree_potential):
        returns PE = 1/2 sum m phi, writes phi into `phi` when given."""
        ptr = _phi_arg(phi, d_particles.count)
        s = d_particles.struct()
        pe = C.c_double()
        check(self.ctx._lib.nbody_hip_tree_potential(self._h, C.byref(s), theta, G, eps, ptr, C.byref(pe)))
        return pe.value

    def computeField(self, points, theta: float, G: float, eps: float, out=None) -> torch.Tensor:
        """{ax, ay, az, phi} of the tree as built at `points` (nbody_hip_tree_field): the force walk's interaction list
        for each position, without a self-skip, at the multipole order of the last build.  [M, 4]; fills `out` when
        given."""
        p4, out = _field_args(points, out)
        check(self.ctx._lib.nbody_hip_tree_field(self._h, p4.data_ptr(), p4.shape[0], theta, G, eps, out.data_ptr()))
        return out

    def stats(self):
        nc, rm, nv = C.c_int(), C.c_float(), C.c_ulonglong()
        lb = (C.c_int * 24)()  # NBODY_HIP_TREE_LEVELS
        check(self.ctx._lib.nbody_hip_tree_stats(self._h, C.byref(nc), C.byref(rm), C.byref(nv),
                                                 C.byref(lb)))
        return {"node_count": nc.value, "root_mass": rm.value, "nodes_visited": nv.value,
                "level_base": list(lb)}

    def idLayout(self):
        """(aligned, id_base) of the last build (nbody_hip_tree_id_layout): whether the sibling groups were padded to
        even ids, and the first id of every level in the numbering the walks use (holes included); stats()["level_base"]
        is the compacted numbering of copyNodesToHost."""
        al = C.c_int()
        ids = (C.c_int * 24)()  # NBODY_HIP_TREE_LEVELS
        check(self.ctx._lib.nbody_hip_tree_id_layout(self._h, C.byref(al), C.byref(ids)))
        return bool(al.value), list(ids)

    def getNodeCount(self) -> int:
        return self.stats()["node_count"]

    def getMaxDepth(self) -> int:
        """deepest level that holds nodes (ref: BarnesHutTree::getMaxDepth, barnes_hut_tree.hpp:43: the depth the
        insertion reached)"""
        lb = self.stats()["level_base"]
        return max([l - 1 for l in range(1, len(lb)) if lb[l] > lb[l - 1]] + [0])

    def copyNodesToHost(self):
        n = self.getNodeCount()
        nodes = np.zeros(n, dtype=OCTREE_NODE_DTYPE)
        order = np.empty(self._count, np.int32)
        check(self.ctx._lib.nbody_hip_tree_copy_nodes(self._h, nodes.ctypes.data, n, order.ctypes.data))
        self.h_nodes_ = nodes
        self.sorted_indices_ = order
        return nodes

    def getNodes(self):
        return self.h_nodes_

    def verifyTreeStructure(self) -> bool:
        return self.getNodeCount() > 0  # force_barnes_hut.cu:505-509

    def verifyMassConservation(self, h_particles: ParticleData) -> bool:
        """force_barnes_hut.cu:511-519: |sum m - root mass| < 0.001 sum m (fp32 sum)."""
        total = np.float32(0)
        for v in h_particles.mass[: h_particles.count]:
            total = np.float32(total + v)
        root = np.float32(self.stats()["root_mass"])
        return bool(abs(total - root) < np.float32(0.001) * total)


class BarnesHutCalculator(ForceCalculator):
    """force_calculator.hpp:136-165 / force_barnes_hut.cu:521-532: the tree is created lazily at
    the first computeForces and sized from that particle count."""

    def __init__(self, theta: float = 0.5, ctx: Context | None = None):
        super().__init__(ctx)
        self.tree_ = None
        self.theta_ = float(theta)
        self.multipole_order_ = 1

    def _tree(self, count: int) -> BarnesHutTree:
        if self.tree_ is None:
            self.tree_ = BarnesHutTree(count, self.ctx)
            if self.multipole_order_ != 1:
                self.tree_.setMultipoleOrder(self.multipole_order_)
        return self.tree_

    def computeForces(self, d_particles: ParticleData):
        self._tree(d_particles.count).build(d_particles)
        self.tree_.computeForces(d_particles, self.theta_, self.G_, self.softening_eps_)

    def computePotential(self, d_particles: ParticleData, phi=None) -> float:
        _phi_arg(phi, d_particles.count)
        self._tree(d_particles.count).build(d_particles)
        return self.tree_.computePotential(d_particles, self.theta_, self.G_, self.softening_eps_, phi)

    def computeField(self, d_particles: ParticleData, points, out=None) -> torch.Tensor:
        p4, out = _field_args(points, out)
        self._tree(d_particles.count).build(d_particles)
        return self.tree_.computeField(p4, self.theta_, self.G_, self.softening_eps_, out)

    def _graph_key(self):
        return (self.G_, self.softening_eps_, self.theta_, id(self.tree_), getattr(self.tree_, "_params", None),
                self.multipole_order_)

    def setMultipoleOrder(self, order: int):
        """Multipole order of the tree (1 = monopoles, the default; 2 = monopoles + quadrupoles): applies to the tree
        now or when it is created, from the next computeForces / computePotential / Integrator step."""
        if self.tree_ is not None:
            self.tree_.setMultipoleOrder(order)
        elif int(order) not in (1, 2):
            raise ValidationException("multipole order must be 1 or 2")
        self.multipole_order_ = int(order)

    def getMultipoleOrder(self) -> int:
        return self.multipole_order_

    def getMethod(self):
        return ForceMethod.BARNES_HUT

    def setTheta(self, theta):
        self.theta_ = float(theta)

    def getTheta(self):
        return self.theta_

    def getTree(self):
        return self.tree_


def createForceCalculator(method: ForceMethod, config: SimulationConfig,
                          ctx: Context | None = None) -> ForceCalculator:
    """force_spatial_hash.cu:380-401: unknown enumerators fall back to Direct."""
    if method == ForceMethod.BARNES_HUT:
        calc = BarnesHutCalculator(config.barnes_hut_theta, ctx)
        calc.setGravitationalConstant(config.G)
        calc.setSofteningParameter(config.softening)
        return calc
    if method == ForceMethod.SPATIAL_HASH:
        calc = SpatialHashCalculator(config.spatial_hash_cell_size, config.spatial_hash_cutoff, ctx)
        calc.setGravitationalConstant(config.G)
        calc.setSofteningParameter(config.softening)
        return calc
    calc = DirectForceCalculator(config.cuda_block_size, ctx)
    calc.setGravitationalConstant(config.G)
    calc.setSofteningParameter(config.softening)
    return calc


# ---- integrator ------------------------------------------------------------------------------

class Integrator:
    """integrator.hpp:51-150 / integrator.cu:224-293."""

    def __init__(self, block_size: int = 256, ctx: Context | None = None):
        self.block_size_ = block_size
        self._ctx = ctx

    @property
    def ctx(self) -> Context:
        if self._ctx is None:
            self._ctx = default_context()
        return self._ctx

    @staticmethod
    def _fusable(force_calc) -> bool:
        return (type(force_calc) is DirectForceCalculator
                and isinstance(force_calc.block_size_, int) and 1 <= force_calc.block_size_ <= 1024)

    def integrate(self, d_particles: ParticleData, force_calc: ForceCalculator, dt: float):
        # integrator.cu:224-238.  The extension point is the virtual computeForces
        # (force_calculator.hpp:36-58): the fused launch sequence is taken only for exactly the
        # engine's own DirectForceCalculator, on that calculator's context, and only with a block
        # size its computeForces would accept (otherwise the call below reports it).
        if self._fusable(force_calc):
            s = d_particles.struct()
            fctx = force_calc.ctx
            check(fctx._lib.nbody_hip_integrate_direct(
                fctx.handle, C.byref(s), force_calc.G_, force_calc.softening_eps2_, dt, 1))
            return
        # exactly the engine's own tree / grid calculators (same rule): the drift rides on the packing pass of
        # their build (one pass over the bodies less); same arithmetic, same results
        if type(force_calc) is BarnesHutCalculator and force_calc.tree_ is not None:
            force_calc.tree_.driftBuild(d_particles, dt)
            force_calc.tree_.computeForces(d_particles, force_calc.theta_, force_calc.G_, force_calc.softening_eps_)
            self.updateVelocities(d_particles, dt)
            return
        if type(force_calc) is SpatialHashCalculator and force_calc.grid_ is not None:
            force_calc.grid_.driftBuild(d_particles, dt)
            force_calc.grid_.computeForces(d_particles, force_calc.cutoff_radius_, force_calc.G_,
                                           force_calc.softening_eps_)
            self.updateVelocities(d_particles, dt)
            return
        s = d_particles.struct()  # a_old <- a and the position update in one pass
        check(self.ctx._lib.nbody_hip_drift(self.ctx.handle, C.byref(s), dt))
        force_calc.computeForces(d_particles)
        self.updateVelocities(d_particles, dt)

    def integrate_steps(self, d_particles, force_calc: ForceCalculator, dt: float, steps: int,
                        graph: bool | None = None):
        """`steps` Velocity-Verlet steps queued back to back.  With graph=True the first step runs
        eagerly (it sizes the workspaces), the second is recorded into a hipGraph and the rest replay
        it; the recording is reused while (arrays, count, dt, calculator parameters) stay the same.
        Off by default: measured on MI355X (profiles/r01_step_graph_probe.txt) a replayed step takes
        the same time as the eager one at every size -- the gaps between the small dependent kernels
        are on the GPU side, not in the host's launch calls.  The spatial-hash step reads its grid
        size back every build and always runs eagerly."""
        if steps <= 0:
            return
        if graph is None:
            graph = False
        if graph and (isinstance(force_calc, SpatialHashCalculator) or force_calc.ctx is not self.ctx):
            graph = False  # not capturable / the step's launches would be split over two contexts
        if not graph:
            if self._fusable(force_calc):
                s = d_particles.struct()
                fctx = force_calc.ctx
                check(fctx._lib.nbody_hip_integrate_direct(
                    fctx.handle, C.byref(s), force_calc.G_, force_calc.softening_eps2_, dt, steps))
            else:
                for _ in range(steps):
                    self.integrate(d_particles, force_calc, dt)
            return
        ctx = force_calc.ctx  # the calculator's context is the one the step's launches go to
        key = (d_particles.pos_x.data_ptr(), d_particles.count, float(dt), id(force_calc), force_calc._graph_key(),
               id(ctx))

        def record(steps):
            self._graph, self._graph_for = None, None
            self.integrate(d_particles, force_calc, dt)  # eager: allocations happen here
            steps -= 1
            if steps > 0:
                with ctx.capture() as rec:
                    self.integrate(d_particles, force_calc, dt)
                self._graph, self._graph_for = rec.graph, key
            return steps

        if getattr(self, "_graph_for", None) != key:
            steps = record(steps)
            if steps == 0:
                return
        try:
            self._graph.launch(steps)
        except StateException:
            # stale recording: another system grew a workspace of the shared context, or the tree was
            # re-sized, since it was made (nbody_hip_graph_launch checks the generation) -> record again
            steps = record(steps)
            if steps:
                self._graph.launch(steps)

    def updatePositions(self, d_particles, dt):
        s = d_particles.struct()
        check(self.ctx._lib.nbody_hip_update_positions(self.ctx.handle, C.byref(s), dt))

    def updateVelocities(self, d_particles, dt):
        s = d_particles.struct()
        check(self.ctx._lib.nbody_hip_update_velocities(self.ctx.handle, C.byref(s), dt))

    def storeOldAccelerations(self, d_particles):
        s = d_particles.struct()
        check(self.ctx._lib.nbody_hip_store_accelerations(self.ctx.handle, C.byref(s)))

    def computeKineticEnergy(self, d_particles) -> float:
        s = d_particles.struct()
        out = C.c_float()
        check(self.ctx._lib.nbody_hip_kinetic_energy(self.ctx.handle, C.byref(s), C.byref(out)))
        return out.value

    def computePotentialEnergy(self, d_particles, G, eps) -> float:
        s = d_particles.struct()
        out = C.c_float()
        check(self.ctx._lib.nbody_hip_potential_energy(self.ctx.handle, C.byref(s), G, eps,
                                                       C.byref(out)))
        return out.value

    def computeTotalEnergy(self, d_particles, G, eps) -> float:
        # integrator.cu:291-293: fp32 sum of the two
        return float(np.float32(self.computeKineticEnergy(d_particles)) +
                     np.float32(self.computePotentialEnergy(d_particles, G, eps)))

    def computeKineticEnergyF64(self, d_particles) -> float:
        s = d_particles.struct()
        ke = C.c_double()
        check(self.ctx._lib.nbody_hip_kinetic_energy_f64(self.ctx.handle, C.byref(s), C.byref(ke)))
        return ke.value

    def computeEnergiesF64(self, d_particles, G, eps):
        s = d_particles.struct()
        ke, pe = C.c_double(), C.c_double()
        check(self.ctx._lib.nbody_hip_kinetic_energy_f64(self.ctx.handle, C.byref(s), C.byref(ke)))
        check(self.ctx._lib.nbody_hip_potential_energy_f64(self.ctx.handle, C.byref(s), G, eps,
                                                           C.byref(pe)))
        return ke.value, pe.value

    def setBlockSize(self, size):
        self.block_size_ = size

    def getBlockSize(self):
        return self.block_size_


STATE_PRECISIONS = ("fp32", "extended")

# ---- ensemble diagnostics (nbody_hip_system_diag, include/nbody_hip.h) --------------------------------------------------
# one row per system; the numpy twin of _lib.SystemDiagStruct
SYSTEM_DIAG_DTYPE = np.dtype([("mass", "<f8"), ("com", "<f8", (3,)), ("momentum", "<f8", (3,)), ("ang_mom", "<f8", (3,)),
                              ("kinetic", "<f8"), ("potential", "<f8"), ("min_sep", "<f8"), ("bind_energy", "<f8"),
                              ("bind_a", "<f8"), ("bind_e", "<f8"), ("min_i", "<i4"), ("min_j", "<i4"), ("bind_i", "<i4"),
                              ("bind_j", "<i4"), ("n", "<i4"), ("status", "<i4")])
SYSTEM_DIAG_BYTES = 152
assert SYSTEM_DIAG_DTYPE.itemsize == SYSTEM_DIAG_BYTES == C.sizeof(_lib.SystemDiagStruct)


# ---- ensemble events (nbody_hip_batch_event_t, include/nbody_hip.h) -----------------------------------------------------
# one row per system; the numpy twin of _lib.BatchEventStruct.  "None": d2 = +inf, i = j = BATCH_EVENT_NONE.
BATCH_EVENT_DTYPE = np.dtype([("stopped", "<u4"), ("reserved", "<u4"), ("macro_steps_done", "<u8"), ("closest_d2", "<f4"),
                              ("closest_i", "<u4"), ("closest_j", "<u4"), ("closest_tick", "<u4"), ("closest_macro", "<u8"),
                              ("contact_d2", "<f4"), ("contact_i", "<u4"), ("contact_j", "<u4"), ("contact_tick", "<u4"),
                              ("contact_macro", "<u8")])
BATCH_EVENT_NONE = 0xFFFFFFFF
STOPPED_RUNNING, STOPPED_CONTACT, STOPPED_BUDGET = 0, 1, 2
assert BATCH_EVENT_DTYPE.itemsize == 64 == C.sizeof(_lib.BatchEventStruct)

# ---- ensemble outcomes (nbody_hip_batch_outcome_t, include/nbody_hip.h) ---------------------------------------------------
# one row per system; the numpy twin of _lib.BatchOutcomeStruct.  "None": escaped = 0, escaper = BATCH_EVENT_NONE, the rest 0.
BATCH_OUTCOME_DTYPE = np.dtype([("escaped", "<u4"), ("escaper", "<u4"), ("macro", "<u8"), ("r", "<f8"), ("vr", "<f8"),
                                ("energy", "<f8"), ("rest_mass", "<f8"), ("reserved", "<f8"), ("reserved2", "<f8")])
BATCH_OUTCOMES_STOP_ON_ESCAPE = _lib.BATCH_OUTCOMES_STOP_ON_ESCAPE
BATCH_STOPPED_ESCAPE = _lib.BATCH_STOPPED_ESCAPE
BatchOutcomeStruct = _lib.BatchOutcomeStruct
assert BATCH_OUTCOME_DTYPE.itemsize == 64 == C.sizeof(_lib.BatchOutcomeStruct)

# ---- ensemble hierarchies (nbody_hip_batch_hierarchy_t, nbody_hip_batch_node_t, include/nbody_hip.h) -----------------------
# one record per system and 2 n node slots per system, from slot 2 offsets[s]; the numpy twins of _lib.BatchHierarchyStruct
# and _lib.BatchNodeStruct.  "None": all 0 but min_sep = +inf and min_p = min_q = BATCH_EVENT_NONE; every slot zero.
BATCH_HIERARCHY_DTYPE = np.dtype([("resolved", "<u4"), ("top_count", "<u4"), ("macro", "<u8"), ("node_count", "<u4"),
                                  ("largest", "<u4"), ("min_sep", "<f8"), ("min_p", "<u4"), ("min_q", "<u4"),
                                  ("reserved", "<f8", (3,))])
BATCH_NODE_DTYPE = np.dtype([("left", "<u4"), ("right", "<u4"), ("parent", "<u4"), ("bodies", "<u4"), ("mass", "<f8"),
                             ("a", "<f8"), ("e", "<f8"), ("r", "<f8"), ("energy", "<f8"), ("reserved", "<f8")])
BATCH_HIERARCHY_STOP_ON_RESOLVED = _lib.BATCH_HIERARCHY_STOP_ON_RESOLVED
BATCH_HIERARCHY_MAX = _lib.BATCH_HIERARCHY_MAX
BATCH_STOPPED_RESOLVED = _lib.BATCH_STOPPED_RESOLVED
BatchHierarchyStruct = _lib.BatchHierarchyStruct
BatchNodeStruct = _lib.BatchNodeStruct
assert BATCH_HIERARCHY_DTYPE.itemsize == 64 == C.sizeof(_lib.BatchHierarchyStruct)
assert BATCH_NODE_DTYPE.itemsize == 64 == C.sizeof(_lib.BatchNodeStruct)

# ---- ensemble mergers (nbody_hip_batch_merger_state_t, nbody_hip_batch_merger_t, include/nbody_hip.h) -----------------------
# one state row per system; one log row per merger (EnsembleMergers.log() adds the system column in front of the numpy twin
# of _lib.BatchMergerStruct).  moved_from = BATCH_EVENT_NONE: no body moved; the id of a dead slot is BATCH_EVENT_NONE.
BATCH_MERGER_STATE_DTYPE = np.dtype([("n_live", "<u4"), ("n_mergers", "<u4"), ("flags", "<u4"), ("reserved", "<u4", (5,))])
_BATCH_MERGER_ENTRY = [("slot_a", "<u4"), ("slot_b", "<u4"), ("id_a", "<u4"), ("id_b", "<u4"), ("moved_from", "<u4"),
                       ("contact_tick", "<u4"), ("contact_macro", "<u8"), ("contact_d2", "<f4"), ("radius", "<f4"),
                       ("mass", "<f8"), ("delta_ke", "<f8"), ("delta_pe", "<f8")]
BATCH_MERGER_ENTRY_DTYPE = np.dtype(_BATCH_MERGER_ENTRY)
BATCH_MERGER_DTYPE = np.dtype([("system", "<u4")] + _BATCH_MERGER_ENTRY)
BATCH_MERGERS_ON = _lib.BATCH_MERGERS_ON
BATCH_MERGER_BAD_RECORD = _lib.BATCH_MERGER_BAD_RECORD
BatchMergerStateStruct = _lib.BatchMergerStateStruct
BatchMergerStruct = _lib.BatchMergerStruct
assert BATCH_MERGER_STATE_DTYPE.itemsize == 32 == C.sizeof(_lib.BatchMergerStateStruct)
assert BATCH_MERGER_ENTRY_DTYPE.itemsize == 64 == C.sizeof(_lib.BatchMergerStruct)


def hierarchy_string(nodes, n: int) -> str:
    """The canonical string of the forest in one system's node table (BATCH_NODE_DTYPE rows, or anything indexable by
    "left", "right", "parent"; the first n rows are the bodies): a leaf prints as its index, a composite as "[A B]" with
    the child that holds the lowest body index first; the top nodes (parent = BATCH_EVENT_NONE) are ordered by their
    lowest body index and joined by one space.  "[0 2] 1" is an exchange from "[0 1] 2", "0 1 2" an ionisation.  Two
    forests are the same outcome exactly when their strings are equal.  Rows that are all zero (at and above the node
    count) are not nodes.  Needs no GPU."""
    n = int(n)
    left, right, parent = (np.asarray(nodes[k]).astype(np.int64) for k in ("left", "right", "parent"))
    if n < 1 or left.shape[0] < n:
        raise ValidationException(f"a node table of {n} bodies has at least {n} rows, got {left.shape[0]}")
    count = n
    while count < left.shape[0] and not (left[count] == 0 and right[count] == 0):
        count += 1

    def walk(k):  # -> (lowest body index, text)
        if k < n:
            return k, str(k)
        if not (0 <= left[k] < k and 0 <= right[k] < k):
            raise ValidationException(f"node {k} has children {int(left[k])} and {int(right[k])}: not a node table")
        a, b = sorted((walk(int(left[k])), walk(int(right[k]))))
        return a[0], f"[{a[1]} {b[1]}]"

    tops = sorted(walk(k) for k in range(count) if parent[k] == BATCH_EVENT_NONE)
    return " ".join(t for _, t in tops)


def system_diag_tensor(n_systems: int, device) -> torch.Tensor:
    """A zeroed device buffer for n_systems structs ([n_systems, 152] uint8): the `out` of the *_into forms."""
    return torch.zeros((int(n_systems), SYSTEM_DIAG_BYTES), dtype=torch.uint8, device=device)


def system_diag_array(out: torch.Tensor) -> np.ndarray:
    """The structs of a buffer the *_into forms wrote, as a numpy structured array (SYSTEM_DIAG_DTYPE), one row per
    system.  The copy blocks (torch orders it after the launches on the current stream)."""
    return out.detach().cpu().contiguous().numpy().reshape(-1).view(SYSTEM_DIAG_DTYPE).copy()


def _diag_out(out, n_systems: int, device):
    """the `out` tensor of a *_into form, checked: n_systems * 152 bytes, contiguous, on the device"""
    if not isinstance(out, torch.Tensor):
        raise ValidationException("out must be a torch tensor (system_diag_tensor makes one)")
    if out.device != device:
        raise ValidationException(f"out must live on {device}, got {out.device}")
    if not out.is_contiguous() or out.numel() * out.element_size() != n_systems * SYSTEM_DIAG_BYTES:
        raise ValidationException(f"out must be contiguous and hold {n_systems} x {SYSTEM_DIAG_BYTES} bytes, got "
                                  f"{out.numel() * out.element_size()} bytes")
    if out.data_ptr() % 8:
        raise ValidationException("out must be 8-byte aligned")
    return out


def _diag_lo(name, lo, count: int, device):
    if lo is None:
        return None
    if (not isinstance(lo, torch.Tensor) or lo.dtype != torch.float32 or tuple(lo.shape) != (count, 4)
            or not lo.is_contiguous()):
        raise ValidationException(f"{name} must be a contiguous float32 tensor of shape ({count}, 4)")
    if lo.device != device:
        raise ValidationException(f"{name} must live on the device of the particle data")
    return lo.data_ptr()


def _diag_offsets(offsets, device) -> torch.Tensor:
    """offsets as an int64 device tensor of B + 1 >= 1 entries (a host array is uploaded; the VALUES are checked on the
    device, per system)"""
    if isinstance(offsets, torch.Tensor):
        if offsets.dtype != torch.int64 or offsets.dim() != 1 or not offsets.is_contiguous() or offsets.numel() < 1:
            raise ValidationException("offsets must be a contiguous one-dimensional int64 tensor of B + 1 entries")
        if offsets.device != device:
            raise ValidationException("offsets must live on the device of the particle data")
        return offsets
    a = np.asarray(offsets)
    if a.ndim != 1 or a.size < 1:
        raise ValidationException(f"offsets must be a one-dimensional array of B + 1 entries, got shape {a.shape}")
    if a.dtype.kind not in "iu":
        raise ValidationException(f"offsets must be integers, got dtype {a.dtype}")
    if (a.dtype.kind == "i" and (a < 0).any()) or (a.size and int(a.max()) > 2 ** 62):
        raise ValidationException("offsets must be in [0, 2^62]")
    return torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(device)


def systems_diagnostics_into(ctx: Context, d_particles: ParticleData, offsets, G: float, eps: float, out: torch.Tensor,
                             pos_lo=None, vel_lo=None):
    """nbody_hip_systems_diagnostics, asynchronous: the struct of system s = bodies [offsets[s], offsets[s + 1]) into
    row s of `out` (system_diag_tensor).  offsets: an int64 DEVICE tensor of B + 1 entries (then nothing is allocated
    and the call can be recorded into a step graph) or a host array (uploaded first).  pos_lo / vel_lo: [N, 4] float32
    device tensors {lx, ly, lz, 0} or None.  Takes eps (not eps^2).  Returns `out`."""
    validateSoftening(eps)
    dev = d_particles.pos_x.device
    off = _diag_offsets(offsets, dev)
    n_systems = off.numel() - 1
    _diag_out(out, n_systems, dev)
    if n_systems == 0:
        return out
    pl = _diag_lo("pos_lo", pos_lo, d_particles.count, dev)
    vl = _diag_lo("vel_lo", vel_lo, d_particles.count, dev)
    s = d_particles.struct()
    check(ctx._lib.nbody_hip_systems_diagnostics(ctx.handle, C.byref(s), pl, vl, off.data_ptr(), n_systems, G, eps,
                                                 out.data_ptr()))
    return out


def systems_diagnostics(ctx: Context, d_particles: ParticleData, offsets, G: float, eps: float, pos_lo=None, vel_lo=None):
    """Per-system fp64 diagnostics of any particle data (nbody_hip_systems_diagnostics): a numpy structured array
    (SYSTEM_DIAG_DTYPE), one row per system -- mass, com, momentum, ang_mom, kinetic, potential, min_sep, the most bound
    pair (bind_energy, bind_a, bind_e), the system-local pair indices, n and status (1: the offsets of that system are
    not a legal range).  Blocks for the copy."""
    dev = d_particles.pos_x.device
    off = _diag_offsets(offsets, dev)
    out = system_diag_tensor(off.numel() - 1, dev)
    systems_diagnostics_into(ctx, d_particles, off, G, eps, out, pos_lo, vel_lo)
    ctx.synchronize()
    return system_diag_array(out)


# ---- group properties (nbody_hip_group_props, include/nbody_hip_group_props.h) ------------------------------------------------
# one row per group; the numpy twin of _lib.GroupPropsStruct
GROUP_PROPS_DTYPE = np.dtype([("mass", "<f8"), ("com", "<f8", (3,)), ("vel", "<f8", (3,)), ("ang_mom", "<f8", (3,)),
                              ("kinetic", "<f8"), ("inertia", "<f8", (6,)), ("r_max", "<f8"), ("potential", "<f8"),
                              ("phi_min", "<f8"), ("n", "<i4"), ("label", "<i4"), ("r_max_body", "<i4"),
                              ("phi_min_body", "<i4"), ("status", "<i4"), ("reserved", "<i4", (3,))])
GROUP_PROPS_BYTES = 192
assert GROUP_PROPS_DTYPE.itemsize == GROUP_PROPS_BYTES == C.sizeof(_lib.GroupPropsStruct)


def group_props_tensor(n_groups: int, device) -> torch.Tensor:
    """A zeroed device buffer for n_groups structs ([n_groups, 192] uint8): the `out` of the *_into forms."""
    return torch.zeros((int(n_groups), GROUP_PROPS_BYTES), dtype=torch.uint8, device=device)


def group_props_array(out: torch.Tensor) -> np.ndarray:
    """The structs of a buffer the *_into forms wrote, as a numpy structured array (GROUP_PROPS_DTYPE), one row per
    group.  The copy blocks (torch orders it after the launches on the current stream)."""
    return out.detach().cpu().contiguous().numpy().reshape(-1).view(GROUP_PROPS_DTYPE).copy()


def _group_ints(name, a, device) -> torch.Tensor:
    """offsets / members as a contiguous one-dimensional int32 device tensor (a host array is uploaded; the VALUES are
    checked on the device, per group)"""
    if isinstance(a, torch.Tensor):
        if a.dtype != torch.int32 or a.dim() != 1 or not a.is_contiguous():
            raise ValidationException(f"{name} must be a contiguous one-dimensional int32 tensor")
        if a.device != device:
            raise ValidationException(f"{name} must live on the device of the particle data")
        return a
    h = np.asarray(a)
    if h.ndim != 1 or (h.size and h.dtype.kind not in "iu"):
        raise ValidationException(f"{name} must be a one-dimensional array of integers, got shape {h.shape} dtype {h.dtype}")
    if h.size and (int(h.max()) > 2 ** 31 - 1 or int(h.min()) < -2 ** 31):
        raise ValidationException(f"{name} must fit 32-bit integers")
    return torch.from_numpy(np.ascontiguousarray(h, np.int32)).to(device)


def groups_properties_into(ctx: Context, d_particles: ParticleData, offsets, members, out: torch.Tensor, phi=None):
    """nbody_hip_groups_properties, asynchronous: the struct of group g = bodies members[offsets[g] : offsets[g + 1]] into
    row g of `out` (group_props_tensor).  offsets (G + 1 entries) and members: int32 DEVICE tensors (then nothing is
    allocated here, and the call can be recorded into a step graph once one of these sizes has run eagerly) or host
    arrays (uploaded first).  phi: a float32 device tensor of d_particles.count entries or None.  Returns `out`."""
    dev = d_particles.pos_x.device
    off = _group_ints("offsets", offsets, dev)
    mem = _group_ints("members", members, dev)
    if off.numel() < 1:
        raise ValidationException("offsets must hold G + 1 >= 1 entries")
    n_groups = off.numel() - 1
    if not isinstance(out, torch.Tensor):
        raise ValidationException("out must be a torch tensor (group_props_tensor makes one)")
    if out.device != dev:
        raise ValidationException(f"out must live on {dev}, got {out.device}")
    if not out.is_contiguous() or out.numel() * out.element_size() != n_groups * GROUP_PROPS_BYTES:
        raise ValidationException(f"out must be contiguous and hold {n_groups} x {GROUP_PROPS_BYTES} bytes, got "
                                  f"{out.numel() * out.element_size()} bytes")
    if out.data_ptr() % 8:
        raise ValidationException("out must be 8-byte aligned")
    ptr = _phi_arg(phi, d_particles.count)
    if n_groups == 0:
        return out
    s = d_particles.struct()
    check(ctx._lib.nbody_hip_groups_properties(ctx.handle, C.byref(s), off.data_ptr(), mem.data_ptr() if mem.numel() else None,
                                               n_groups, mem.numel(), ptr, out.data_ptr()))
    return out


def groups_properties(ctx: Context, d_particles: ParticleData, offsets, members, phi=None) -> np.ndarray:
    """Per-group fp64 properties of any catalogue over any particle data (nbody_hip_groups_properties): a numpy structured
    array (GROUP_PROPS_DTYPE), one row per group; status 1 (with n = 0 and zeros): the offsets of that group are not a
    legal range or one of its member indices is outside the particle data.  Blocks for the copy."""
    dev = d_particles.pos_x.device
    off = _group_ints("offsets", offsets, dev)
    out = group_props_tensor(max(off.numel() - 1, 0), dev)
    groups_properties_into(ctx, d_particles, off, members, out, phi)
    ctx.synchronize()
    return group_props_array(out)


# ---- radial profiles (nbody_hip_radial_group / nbody_hip_radial_shell, include/nbody_hip_radial.h) ----------------------------
RADIAL_GROUP_DTYPE = np.dtype([("mass", "<f8"), ("r_max", "<f8"), ("n", "<i4"), ("status", "<i4"), ("reserved", "<i4", (2,))])
RADIAL_SHELL_DTYPE = np.dtype([("radius", "<f8"), ("enclosed_mass", "<f8"), ("mass", "<f8"), ("m_vr", "<f8"),
                               ("m_vr2", "<f8"), ("m_vt2", "<f8"), ("count", "<i4"), ("enclosed_count", "<i4"),
                               ("reserved", "<i4", (2,))])
RADIAL_GROUP_BYTES, RADIAL_SHELL_BYTES, RADIAL_MAX_CUTS = 32, 64, 16
RADIAL_MODES = {"mass": 0, "number": 1, "radius": 2}
assert RADIAL_GROUP_DTYPE.itemsize == RADIAL_GROUP_BYTES == C.sizeof(_lib.RadialGroupStruct)
assert RADIAL_SHELL_DTYPE.itemsize == RADIAL_SHELL_BYTES == C.sizeof(_lib.RadialShellStruct)


def radial_tensors(n_groups: int, n_cuts: int, device):
    """Zeroed device buffers for the two outputs of the *_into form: ([n_groups, 32], [n_groups * n_cuts, 64]) uint8."""
    return (torch.zeros((int(n_groups), RADIAL_GROUP_BYTES), dtype=torch.uint8, device=device),
            torch.zeros((int(n_groups) * int(n_cuts), RADIAL_SHELL_BYTES), dtype=torch.uint8, device=device))


def radial_arrays(groups: torch.Tensor, shells: torch.Tensor, n_cuts: int):
    """The structs of the buffers the *_into form wrote: (groups [G] RADIAL_GROUP_DTYPE, shells [G, n_cuts]
    RADIAL_SHELL_DTYPE).  The copy blocks."""
    g = groups.detach().cpu().contiguous().numpy().reshape(-1).view(RADIAL_GROUP_DTYPE).copy()
    s = shells.detach().cpu().contiguous().numpy().reshape(-1).view(RADIAL_SHELL_DTYPE).copy()
    return g, s.reshape(len(g), int(n_cuts))


def _radial_cuts(cuts, mode):
    """-> (the cuts as a contiguous float64 host array, the mode's number); the library checks their values"""
    if isinstance(mode, str):
        if mode not in RADIAL_MODES:
            raise ValidationException(f"mode must be one of {sorted(RADIAL_MODES)}, got {mode!r}")
        mode = RADIAL_MODES[mode]
    if isinstance(cuts, torch.Tensor):
        cuts = cuts.detach().cpu().numpy()
    arr = np.ascontiguousarray(np.atleast_1d(np.asarray(cuts, np.float64)))
    if arr.ndim != 1:
        raise ValidationException("cuts must be a one-dimensional sequence of numbers")
    return arr, int(mode)


def _radial_centres(name, a, n_groups, device):
    """centres / bulk velocities as a contiguous float64 device tensor of 3 * n_groups elements (a host array is
    uploaded); None stays None"""
    if a is None:
        return None
    if not isinstance(a, torch.Tensor):
        a = torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).to(device)
    if a.dtype != torch.float64 or a.device != torch.device(device) or not a.is_contiguous() or a.numel() != 3 * n_groups:
        raise ValidationException(f"{name} must be a contiguous float64 tensor of {n_groups} x 3 elements on {device}")
    return a


def groups_radial_profile_into(ctx: Context, d_particles: ParticleData, offsets, members, centres, cuts, groups: torch.Tensor,
                               shells: torch.Tensor, mode="mass", vels=None, sorted_members=None, sorted_q=None):
    """nbody_hip_groups_radial_profile, asynchronous: the group structs into `groups` and the shell rows (row g * n_cuts +
    c) into `shells` (radial_tensors makes both).  offsets (G + 1 entries, ORDERED) and members: int32 device tensors
    or host arrays (uploaded first); members None: the identity list (offsets [0, count] is all bodies as one group).
    centres, vels: [G, 3] float64 device tensors or host arrays; vels None: zeros.  cuts: up to 16 numbers, strictly
    ascending -- mass or number fractions in (0, 1], or radii >= 0 -- for mode "mass" | "number" | "radius".
    sorted_members (int32) / sorted_q (float32): optional device tensors of n_members elements for the radial order.
    Reads nothing back.  Returns (groups, shells)."""
    dev = d_particles.pos_x.device
    off = _group_ints("offsets", offsets, dev)
    mem = None if members is None else _group_ints("members", members, dev)
    if off.numel() < 1:
        raise ValidationException("offsets must hold G + 1 >= 1 entries")
    n_groups = off.numel() - 1
    n_members = d_particles.count if mem is None else mem.numel()
    cuts_arr, mode_id = _radial_cuts(cuts, mode)
    cen, vel = _radial_centres("centres", centres, n_groups, dev), _radial_centres("vels", vels, n_groups, dev)
    if cen is None:
        raise ValidationException("centres must be given")
    for name, t, rows, width in (("groups", groups, n_groups, RADIAL_GROUP_BYTES),
                                 ("shells", shells, n_groups * cuts_arr.size, RADIAL_SHELL_BYTES)):
        if not isinstance(t, torch.Tensor) or t.device != dev or not t.is_contiguous() or t.data_ptr() % 8 \
                or t.numel() * t.element_size() != rows * width:
            raise ValidationException(f"{name} must be a contiguous, 8-byte aligned tensor of {rows} x {width} bytes on {dev} "
                                      "(radial_tensors makes one)")
    for name, t, dt in (("sorted_members", sorted_members, torch.int32), ("sorted_q", sorted_q, torch.float32)):
        if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == dt and t.device == dev and t.is_contiguous()
                                  and t.numel() == n_members):
            raise ValidationException(f"{name} must be a contiguous {dt} tensor of {n_members} elements on {dev}")
    s = d_particles.struct()
    check(ctx._lib.nbody_hip_groups_radial_profile(
        ctx.handle, C.byref(s), off.data_ptr(), None if mem is None or not mem.numel() else mem.data_ptr(), n_groups,
        n_members, cen.data_ptr() if n_groups else None, None if vel is None or not n_groups else vel.data_ptr(),
        cuts_arr.ctypes.data, cuts_arr.size, mode_id, groups.data_ptr() if n_groups else None,
        shells.data_ptr() if n_groups else None, None if sorted_members is None else sorted_members.data_ptr(),
        None if sorted_q is None else sorted_q.data_ptr()))
    return groups, shells


def groups_radial_profile(ctx: Context, d_particles: ParticleData, offsets, members, centres, cuts, mode="mass", vels=None,
                          sorted_members=None, sorted_q=None):
    """Lagrangian radii and shell moments of the groups of any ordered catalogue about `centres`
    (nbody_hip_groups_radial_profile): -> (groups [G] RADIAL_GROUP_DTYPE -- mass, r_max, n, status --, shells
    [G, n_cuts] RADIAL_SHELL_DTYPE -- radius, enclosed_mass, mass, m_vr, m_vr2, m_vt2, count, enclosed_count).  status
    1: the catalogue is not ordered (every group), the group is empty or has a member index outside the particle data;
    2: a NaN distance.  Blocks for the copy."""
    dev = d_particles.pos_x.device
    off = _group_ints("offsets", offsets, dev)
    cuts_arr, _ = _radial_cuts(cuts, mode)
    groups, shells = radial_tensors(max(off.numel() - 1, 0), cuts_arr.size, dev)
    groups_radial_profile_into(ctx, d_particles, off, members, centres, cuts_arr, groups, shells, mode, vels, sorted_members,
                               sorted_q)
    ctx.synchronize()
    return radial_arrays(groups, shells, cuts_arr.size)


# ---- density centre (nbody_hip_density_centre_t, include/nbody_hip_neighbours.h) ---------------------------------------------
DENSITY_CENTRE_DTYPE = np.dtype([("centre", "<f8", (3,)), ("core_radius", "<f8"), ("rho_sum", "<f8"), ("rho2_sum", "<f8"),
                                 ("n", "<i4"), ("status", "<i4"), ("reserved", "<i4", (2,))])
DENSITY_CENTRE_BYTES = 64
assert DENSITY_CENTRE_DTYPE.itemsize == DENSITY_CENTRE_BYTES == C.sizeof(_lib.DensityCentreStruct)


def density_centre_into(ctx: Context, d_particles: ParticleData, rho: torch.Tensor, out: torch.Tensor, members=None):
    """nbody_hip_density_centre, asynchronous: the struct of the set into `out` (64 bytes of device memory, 8-byte
    aligned).  rho: float64 device tensor of d_particles.count weights; members: None (all bodies) or an int32 device
    tensor / host array of body indices (a slice of a GroupCatalogue's members, for one).  Returns `out`."""
    dev = d_particles.pos_x.device
    if not (isinstance(rho, torch.Tensor) and rho.dtype == torch.float64 and rho.device == dev and rho.is_contiguous()
            and rho.dim() == 1 and rho.numel() == d_particles.count):
        raise ValidationException(f"rho must be a contiguous float64 device tensor of {d_particles.count} elements")
    if not (isinstance(out, torch.Tensor) and out.device == dev and out.is_contiguous()
            and out.numel() * out.element_size() == DENSITY_CENTRE_BYTES and out.data_ptr() % 8 == 0):
        raise ValidationException(f"out must be {DENSITY_CENTRE_BYTES} contiguous, 8-byte aligned bytes on {dev}")
    mem = None if members is None else _group_ints("members", members, dev)
    s = d_particles.struct()
    if mem is not None and mem.numel() == 0:
        mem = torch.zeros(1, dtype=torch.int32, device=dev)  # (a pointer for the empty list: n_members says 0)
        n_members = 0
    else:
        n_members = 0 if mem is None else mem.numel()
    check(ctx._lib.nbody_hip_density_centre(ctx.handle, C.byref(s), rho.data_ptr(), None if mem is None else mem.data_ptr(),
                                            n_members, out.data_ptr()))
    return out


def density_centre(ctx: Context, d_particles: ParticleData, rho: torch.Tensor, members=None):
    """The density centre and core radius of all bodies, or of the bodies `members`, weighted by rho (Casertano and Hut
    1985; nbody_hip_density_centre): a numpy record (DENSITY_CENTRE_DTYPE) -- centre [3], core_radius, rho_sum,
    rho2_sum, n, status (1: a member index outside the particle data, and zeros).  Blocks for the copy."""
    out = torch.zeros(DENSITY_CENTRE_BYTES, dtype=torch.uint8, device=d_particles.pos_x.device)
    density_centre_into(ctx, d_particles, rho, out, members)
    ctx.synchronize()
    return out.cpu().numpy().view(DENSITY_CENTRE_DTYPE)[0].copy()


def _precision_mode(precision) -> int:
    """"fp32" -> 0, "extended" -> 1 (the mode of nbody_hip_hermite_set_precision); anything else is refused"""
    if not isinstance(precision, str) or precision not in STATE_PRECISIONS:
        raise ValidationException(f"state precision must be one of {STATE_PRECISIONS}, got {precision!r}")
    return STATE_PRECISIONS.index(precision)


def _state64(d_particles, pos64, vel64):
    """the two [N, 3] fp64 host arrays of setExtendedState, checked"""
    out = []
    for name, a in (("pos64", pos64), ("vel64", vel64)):
        a = np.ascontiguousarray(a, np.float64)
        if a.shape != (d_particles.count, 3):
            raise ValidationException(f"{name} must have shape ({d_particles.count}, 3), got {a.shape}")
        if not np.isfinite(a).all():
            raise ValidationException(f"{name} must be finite")
        out.append(a)
    return out


class _ExtendedState:
    """What HermiteIntegrator, BlockHermiteIntegrator and BlockHermiteEnsemble share: the handle of the C ABI (_PREFIX
    names its entry points, _KIND its place in the exit hook, _NOUN the word of its messages) with its life cycle, and
    the state-precision methods (nbody_hip_hermite[_block|_batch]_set_precision / get_precision / set_state_f64 /
    get_state_f64).  In "extended" mode the state is X = pos + pos_lo, V = vel + vel_lo with the fp32 residuals on the
    handle; pos_* / vel_* stay the fp32 roundings."""
    _PREFIX = _KIND = _NOUN = ""

    def __init__(self, block_size: int = 256, ctx: Context | None = None):
        self.block_size_ = block_size
        self._ctx = ctx
        self._h = None
        self._capacity = 0
        self._count = 0
        self._precision = 0

    @property
    def ctx(self) -> Context:
        if self._ctx is None:
            self._ctx = default_context()
        return self._ctx

    def _fn(self, name):
        return getattr(self._hctx._lib, self._PREFIX + name)

    def _direct(self, force_calc, method: str) -> "DirectForceCalculator":
        if type(force_calc) is not DirectForceCalculator:
            raise ValueError(f"{type(self).__name__}.{method}: the Hermite scheme is Direct-only -- it needs exactly a "
                             f"DirectForceCalculator (the tree and the grid have no jerk), got "
                             f"{type(force_calc).__name__}")
        return force_calc

    def _require_primed(self, ready: bool = True):
        """StateException before the first priming (no handle yet), or when the class says it is not `ready`"""
        if self._h is None or not ready:
            raise StateException(f"the {self._NOUN} is not primed")

    def _open(self, fctx, outgrown: bool, *sizes) -> bool:
        """The handle on the calculator's context fctx (the one the step's launches go to): a handle on another context,
        or one the data has outgrown, is closed; without one, nbody_hip_hermite*_create(fctx, *sizes) -- sizes[0] is the
        capacity in bodies.  True: the handle is new and the class's settings have to go onto it."""
        if self._h is not None and (fctx is not self._hctx or outgrown):
            self.close()
        if self._h is not None:
            return False
        validateParticleCountRange(sizes[0])
        h = C.c_void_p()
        check(getattr(fctx._lib, self._PREFIX + "create")(fctx.handle, *sizes, C.byref(h)))
        self._h, self._hctx, self._capacity = h, fctx, sizes[0]
        _lib.track(self, self._KIND)
        return True

    def setBlockSize(self, size):
        self.block_size_ = size

    def getBlockSize(self):
        return self.block_size_

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            if self._hctx.handle.value:  # (a closed context has taken its stream with it: nothing left to wait for)
                self._fn("destroy")(self._h)
        self._h = None
        self._capacity = 0

    def __del__(self):
        try:
            if not _lib.finalizing():  # (else: closed by the exit hook _lib.close_all, or the runtime is going down)
                self.close()
        except Exception:
            pass

    def invalidate(self):
        """The caller changed x, v, m, G or eps behind the integrator: the next step primes again (an ensemble: prime
        again before the next advance)."""
        if self._h is not None:
            check(self._fn("invalidate")(self._h))

    def setStatePrecision(self, precision: str):
        """"fp32" (default) or "extended".  A switch re-primes at the next step; switching to "extended" starts with
        residuals 0 (from the rounded state)."""
        mode = _precision_mode(precision)
        if self._h is not None:
            check(self._fn("set_precision")(self._h, mode))
        self._precision = mode

    def getStatePrecision(self) -> str:
        return STATE_PRECISIONS[self._precision]

    def setExtendedState(self, d_particles: ParticleData, pos64, vel64, force_calc=None):
        """X, V as [N, 3] fp64 host arrays: pos_* / vel_* <- their fp32 roundings, the residuals onto the handle (in
        "fp32" mode the rounded state only); the next step primes again.  force_calc: the Direct calculator whose
        context the handle lives on, needed only before the first prime / step.  An ensemble: over all its bodies,
        after setLayout."""
        pos, vel = _state64(d_particles, pos64, vel64)
        if self._h is None or d_particles.count > self._capacity:
            if force_calc is None:
                force_calc = DirectForceCalculator()
            self._handle(d_particles, self._direct(force_calc, "setExtendedState"))
        s = d_particles.struct()
        check(self._fn("set_state_f64")(self._h, C.byref(s), pos.ctypes.data, vel.ctypes.data))
        self._count = d_particles.count

    def getExtendedState(self, d_particles: ParticleData):
        """(X [N, 3], V [N, 3]) in fp64: hi + lo (in "fp32" mode, or before the first step, the arrays widened)"""
        n = d_particles.count
        pos, vel = np.empty((n, 3), np.float64), np.empty((n, 3), np.float64)
        if self._h is None or n > self._capacity:
            for c, k in enumerate("xyz"):
                pos[:, c] = getattr(d_particles, "pos_" + k).cpu().numpy()
                vel[:, c] = getattr(d_particles, "vel_" + k).cpu().numpy()
            return pos, vel
        s = d_particles.struct()
        check(self._fn("get_state_f64")(self._h, C.byref(s), pos.ctypes.data, vel.ctypes.data))
        return pos, vel


class _Energies:
    """The energy methods of Integrator, by delegation to self._energies (the two integrators; an ensemble has none)."""

    def computeKineticEnergy(self, d_particles) -> float:
        return self._energies.computeKineticEnergy(d_particles)

    def computePotentialEnergy(self, d_particles, G, eps) -> float:
        return self._energies.computePotentialEnergy(d_particles, G, eps)

    def computeTotalEnergy(self, d_particles, G, eps) -> float:
        return self._energies.computeTotalEnergy(d_particles, G, eps)

    def computeKineticEnergyF64(self, d_particles) -> float:
        return self._energies.computeKineticEnergyF64(d_particles)

    def computeEnergiesF64(self, d_particles, G, eps):
        return self._energies.computeEnergiesF64(d_particles, G, eps)


class _BlockStepState:
    """What BlockHermiteIntegrator and BlockHermiteEnsemble do alike with the block-step state of their handle
    (nbody_hip_hermite_block_* / _batch_* set_params, state, info)."""

    def setParameters(self, eta: float = 0.02, eta_start: float = 0.01, max_level: int = 16):
        """The accuracy parameters of the level rule and of priming, and the deepest level (an ensemble: for every
        system): they take effect at the next priming."""
        if not (eta > 0 and math.isfinite(eta)):
            raise ValidationException("eta must be positive and finite")
        if not (eta_start > 0 and math.isfinite(eta_start)):
            raise ValidationException("eta_start must be positive and finite")
        if not 0 <= int(max_level) <= 20:
            raise ValidationException(f"max_level must be in [0, 20], got {max_level}")
        self._params = (float(eta), float(eta_start), int(max_level))
        if self._h is not None:
            check(self._fn("set_params")(self._h, *self._params))

    def getState(self) -> dict:
        """dict(levels int32 [N], ticks uint32 [N], want float32 [N], jerk float32 [N, 4]) as numpy arrays, over all
        bodies (StateException before the first priming)."""
        self._require_primed()
        n = self._count
        out = dict(levels=np.empty(n, np.int32), ticks=np.empty(n, np.uint32), want=np.empty(n, np.float32),
                   jerk=np.empty((n, 4), np.float32))
        check(self._fn("state")(self._h, out["levels"].ctypes.data, out["ticks"].ctypes.data, out["want"].ctypes.data,
                                out["jerk"].ctypes.data))
        return out

    def getJerk(self) -> torch.Tensor:
        """{jx, jy, jz, 0} of every body at its own tick as an [N, 4] device tensor."""
        return torch.from_numpy(self.getState()["jerk"]).to(self._hctx.torch_device)

    def _info(self, *args) -> dict:
        """nbody_hip_hermite_block_info_t of self._fn("info")(handle, *args, &info) as a dict"""
        self._require_primed()
        st = _lib.HermiteBlockInfoStruct()
        check(self._fn("info")(self._h, *args, C.byref(st)))
        out = {k: getattr(st, k) for k, _ in st._fields_ if k != "level_steps"}
        out["level_steps"] = list(st.level_steps)
        return out


class HermiteIntegrator(_ExtendedState, _Energies):
    """Fourth-order Hermite integrator (PEC form of Makino & Aarseth 1992) on the Direct force-and-jerk kernel
    (nbody_hip_hermite_*; no reference counterpart -- the reference integrates with Velocity Verlet only).  Direct-only:
    it accepts exactly `type(force_calc) is DirectForceCalculator` (the rule of Integrator._fusable; G and eps come from
    that calculator), because the tree and the grid have no jerk here.  After a step acc_* = a1 and acc_old_* = a as after
    a Velocity-Verlet step; the jerk stays on the handle (getJerk).  (a1, j1) belong to the predicted state, so a run
    continued from a checkpoint agrees with the uninterrupted one to truncation order, not bit for bit."""
    _PREFIX, _KIND, _NOUN = "nbody_hip_hermite_", "hermite", "Hermite integrator"

    def __init__(self, block_size: int = 256, ctx: Context | None = None):
        super().__init__(block_size, ctx)
        self._energies = Integrator(block_size, ctx)

    def _handle(self, d_particles: ParticleData, force_calc):
        if self._open(force_calc.ctx, d_particles.count > self._capacity, d_particles.count) and self._precision:
            check(self._fn("set_precision")(self._h, self._precision))
        return self._h

    def prime(self, d_particles: ParticleData, force_calc):
        """(a, j) at the current state: overwrites acc_*, keeps the jerk on the handle."""
        fc = self._direct(force_calc, "prime")
        h = self._handle(d_particles, fc)
        s = d_particles.struct()
        check(self._hctx._lib.nbody_hip_hermite_prime(h, C.byref(s), fc.G_, fc.softening_eps_))
        self._count = d_particles.count

    def integrate(self, d_particles: ParticleData, force_calc, dt: float):
        self._steps(d_particles, self._direct(force_calc, "integrate"), dt, 1)

    def integrate_steps(self, d_particles: ParticleData, force_calc, dt: float, steps: int):
        """`steps` Hermite steps queued back to back (no host synchronisation); steps <= 0 does nothing."""
        fc = self._direct(force_calc, "integrate_steps")
        if steps <= 0:
            return
        self._steps(d_particles, fc, dt, int(steps))

    def _steps(self, d_particles, fc, dt, steps):
        h = self._handle(d_particles, fc)
        s = d_particles.struct()
        check(self._hctx._lib.nbody_hip_hermite_step(h, C.byref(s), fc.G_, fc.softening_eps_, dt, steps))
        self._count = d_particles.count

    def getJerk(self) -> torch.Tensor:
        """{jx, jy, jz, 0} of the last evaluation as an [N, 4] device tensor (StateException before the first priming)."""
        self._require_primed()
        out = torch.empty((self._count, 4), dtype=torch.float32, device=self._hctx.torch_device)
        check(self._hctx._lib.nbody_hip_hermite_jerk(self._h, out.data_ptr()))
        return out

    def suggestTimeStep(self, eta: float = 0.02) -> float:
        """eta * min |a_i| / |j_i| over the bodies with |j_i| > 0 of the last evaluation: the standard start-up criterion.
        A hint -- the integrator never changes dt itself.  StateException before the first priming."""
        self._require_primed()
        out = C.c_float()
        check(self._hctx._lib.nbody_hip_hermite_suggest_dt(self._h, eta, C.byref(out)))
        return out.value


BLOCK_SCHEDULINGS = ("host", "resident", "auto")
# include/nbody_hip.h: the most bodies the resident form takes, and the body count below which "auto" takes it (the
# measured crossover; 0: never)
HERMITE_BLOCK_RESIDENT_MAX = 4096
HERMITE_BLOCK_RESIDENT_BELOW = 0


def _scheduling_mode(name) -> int:
    """"host" -> 0, "resident" -> 1, "auto" -> 2 (the mode of nbody_hip_hermite_block_set_scheduling)"""
    if not isinstance(name, str) or name not in BLOCK_SCHEDULINGS:
        raise ValidationException(f"block-step scheduling must be one of {BLOCK_SCHEDULINGS}, got {name!r}")
    return BLOCK_SCHEDULINGS.index(name)


class BlockHermiteIntegrator(_ExtendedState, _BlockStepState, _Energies):
    """The Hermite integrator with individual block time steps (nbody_hip_hermite_block_*; no reference counterpart):
    body i steps with dt_max 2^-k_i, its level k_i chosen by the Aarseth criterion, and one call of integrate() advances
    the system by one MACRO step dt_max, after which every body is at the same time.  Direct-only, by the rule of
    HermiteIntegrator: exactly `type(force_calc) is DirectForceCalculator`.  With "host" scheduling (the default) every
    stepping call blocks (the host reads the size of the active set once per block step); with "resident" scheduling
    (setScheduling, systems of up to 4,096 bodies) one workgroup runs the block steps of a macro step inside one launch,
    the stepping calls return at once and can be recorded into a step graph.  Inside a macro step (block_step) the
    arrays of body i hold its state at its own tick."""
    _PREFIX, _KIND, _NOUN = "nbody_hip_hermite_block_", "hermite_block", "block-step Hermite integrator"

    def __init__(self, block_size: int = 256, ctx: Context | None = None):
        super().__init__(block_size, ctx)
        self._params = (0.02, 0.01, 16)
        self._narrow_below = 0
        self._scheduling = 0
        self._energies = Integrator(block_size, ctx)

    def _handle(self, d_particles: ParticleData, force_calc):
        if self._open(force_calc.ctx, d_particles.count > self._capacity, d_particles.count):
            check(self._fn("set_params")(self._h, *self._params))
            check(self._fn("tuning")(self._h, self._narrow_below))
            if self._precision:
                check(self._fn("set_precision")(self._h, self._precision))
            if self._scheduling:
                check(self._fn("set_scheduling")(self._h, self._scheduling))
        return self._h

    def setTuning(self, narrow_below: int = 0):
        """Active sets smaller than narrow_below take the narrow kernel form (0: the measured crossover)."""
        self._narrow_below = int(narrow_below)
        if self._h is not None:
            check(self._hctx._lib.nbody_hip_hermite_block_tuning(self._h, self._narrow_below))

    def setScheduling(self, scheduling: str):
        """Where the block steps are scheduled: "host" (default), "resident" (one workgroup runs whole macro steps; at
        most 4,096 bodies, more is refused by the stepping call) or "auto" (resident below the measured crossover
        HERMITE_BLOCK_RESIDENT_BELOW).  A resident run equals the host-scheduled run with setTuning(1 << 30) bit for
        bit.  Only at a macro boundary (StateException in the middle of a macro step); the priming and the counters stay."""
        mode = _scheduling_mode(scheduling)
        if self._h is not None:
            check(self._hctx._lib.nbody_hip_hermite_block_set_scheduling(self._h, mode))
        self._scheduling = mode

    def getScheduling(self):
        """(the setting, the form the last stepping call ran: "host", "resident" or None before the first one since the
        priming)"""
        if self._h is None:
            return BLOCK_SCHEDULINGS[self._scheduling], None
        mode, form = C.c_int(), C.c_int()
        check(self._hctx._lib.nbody_hip_hermite_block_get_scheduling(self._h, C.byref(mode), C.byref(form)))
        return BLOCK_SCHEDULINGS[mode.value], (None if form.value < 0 else BLOCK_SCHEDULINGS[form.value])

    def prime(self, d_particles: ParticleData, force_calc, dt_max: float):
        """(a, j) at the current state and the start levels for macro steps of dt_max: overwrites acc_*."""
        fc = self._direct(force_calc, "prime")
        h = self._handle(d_particles, fc)
        s = d_particles.struct()
        check(self._hctx._lib.nbody_hip_hermite_block_prime(h, C.byref(s), fc.G_, fc.softening_eps_, dt_max))
        self._count = d_particles.count

    def integrate(self, d_particles: ParticleData, force_calc, dt_max: float):
        """one macro step"""
        self._advance(d_particles, self._direct(force_calc, "integrate"), dt_max, 1)

    def advance(self, d_particles: ParticleData, force_calc, dt_max: float, macro_steps: int):
        """`macro_steps` macro steps; macro_steps <= 0 does nothing."""
        fc = self._direct(force_calc, "advance")
        if macro_steps <= 0:
            return
        self._advance(d_particles, fc, dt_max, int(macro_steps))

    def _advance(self, d_particles, fc, dt_max, macro_steps):
        h = self._handle(d_particles, fc)
        s = d_particles.struct()
        check(self._hctx._lib.nbody_hip_hermite_block_advance(h, C.byref(s), fc.G_, fc.softening_eps_, dt_max,
                                                              macro_steps))
        self._count = d_particles.count

    def block_step(self, d_particles: ParticleData, force_calc, dt_max: float, block_steps: int = 1):
        """Up to `block_steps` single block steps (stops early at a macro boundary)."""
        fc = self._direct(force_calc, "block_step")
        if block_steps <= 0:
            return
        h = self._handle(d_particles, fc)
        s = d_particles.struct()
        check(self._hctx._lib.nbody_hip_hermite_block_step(h, C.byref(s), fc.G_, fc.softening_eps_, dt_max,
                                                           int(block_steps)))
        self._count = d_particles.count

    def getLevels(self) -> np.ndarray:
        self._require_primed()
        out = np.empty(self._count, np.int32)
        check(self._hctx._lib.nbody_hip_hermite_block_state(self._h, out.ctypes.data, None, None, None))
        return out

    def setLevels(self, levels):
        """Test / expert hook: replaces the levels (only at tick 0 of a primed integrator)."""
        self._require_primed()
        lv = np.ascontiguousarray(levels, np.int32)
        if lv.shape != (self._count,):
            raise ValidationException(f"levels must have shape ({self._count},), got {lv.shape}")
        check(self._hctx._lib.nbody_hip_hermite_block_set_levels(self._h, lv.ctypes.data))

    def diagnostics_into(self, d_particles: ParticleData, force_calc, out: torch.Tensor):
        """nbody_hip_hermite_block_diagnostics: the struct of the one system (all bodies, with the residuals in
        "extended" mode; G and eps from force_calc) into `out` (system_diag_tensor(1, device)).  At most 4,096 bodies;
        StateException in the middle of a macro step.  Asynchronous with "host" scheduling; with "resident" scheduling it
        reads the device schedule first."""
        fc = self._direct(force_calc, "diagnostics")
        h = self._handle(d_particles, fc)
        _diag_out(out, 1, d_particles.pos_x.device)
        s = d_particles.struct()
        check(self._hctx._lib.nbody_hip_hermite_block_diagnostics(h, C.byref(s), fc.G_, fc.softening_eps_, out.data_ptr()))
        return out

    def diagnostics(self, d_particles: ParticleData, force_calc) -> np.ndarray:
        """The diagnostics of the system as a structured array of one row (SYSTEM_DIAG_DTYPE).  Blocks for the copy."""
        out = system_diag_tensor(1, d_particles.pos_x.device)
        self.diagnostics_into(d_particles, force_calc, out)
        self._hctx.synchronize()
        return system_diag_array(out)

    def info(self) -> dict:
        """The counters of nbody_hip_hermite_block_info_t since the last priming (StateException before the first)."""
        return self._info()


class BlockHermiteEnsemble(_ExtendedState, _BlockStepState):
    """The block-step Hermite integrator for ENSEMBLES (nbody_hip_hermite_batch_*; no reference counterpart): B
    independent small systems, stored back to back in one ParticleData, advanced by one launch with one workgroup per
    system.  System s is the bodies [offsets[s], offsets[s+1]), 1 to 4,096 of them; no pair is formed across systems;
    eta, eta_start, max_level, the state precision, G and eps are shared, dt_max is per system.  System s of a run equals
    a single-system BlockHermiteIntegrator in "resident" scheduling on those bodies alone bit for bit, whatever its place
    in the batch.  Direct-only, by the rule of HermiteIntegrator: exactly `type(force_calc) is DirectForceCalculator`,
    which supplies G and eps at prime().  prime() and advance() are asynchronous; after one eager advance() a further
    one can be recorded into a step graph."""
    _PREFIX, _KIND, _NOUN = "nbody_hip_hermite_batch_", "hermite_batch", "block-step Hermite ensemble"
    # What setEvents and the companions configure, each the attribute that holds it -> the method that sends it to the
    # handle.  None: not configured.  Sent with the layout, dropped by a new one.
    #   _events     (radii float32 | None, limits uint64 | None, flags)
    #   _outcomes   (escape radii float32, flags), set by an EnsembleOutcomes
    #   _hierarchy  (separation radii float32, kappa, flags), set by an EnsembleHierarchy
    #   _mergers    flags, set by an EnsembleMergers
    _FEATURES = {"_events": "_send_events", "_outcomes": "_send_outcomes", "_hierarchy": "_send_hierarchy",
                 "_mergers": "_send_mergers"}

    def __init__(self, block_size: int = 256, ctx: Context | None = None):
        super().__init__(block_size, ctx)
        self._max_systems = 0
        self._params = (0.02, 0.01, 16)
        self._offsets = None
        self._layout_sent = False
        self._drop_features()

    @staticmethod
    def _check_offsets(offsets) -> np.ndarray:
        """offsets as a contiguous uint64 array of B + 1 >= 2 entries (the values are checked by set_layout)"""
        a = np.asarray(offsets)
        if a.ndim != 1 or a.size < 2:
            raise ValidationException(f"offsets must be a one-dimensional array of B + 1 >= 2 entries, got shape {a.shape}")
        if a.dtype.kind not in "iu":
            raise ValidationException(f"offsets must be integers, got dtype {a.dtype}")
        if a.dtype.kind == "i" and (a < 0).any():
            raise ValidationException("offsets must not be negative")
        return np.ascontiguousarray(a, np.uint64)

    def _handle(self, d_particles: ParticleData, force_calc):
        """the handle on the calculator's context, sized for the layout; the layout goes onto a new handle"""
        if self._offsets is None:
            raise StateException("the ensemble has no layout: call setLayout first")
        total, systems = int(self._offsets.max()), self._offsets.size - 1
        # (a layout the C ABI refuses is refused by set_layout below, with its wording, not by the sizes here)
        cap = max(total, 1)
        ms = min(max(systems, 1), cap)
        if self._open(force_calc.ctx, total > self._capacity or systems > self._max_systems, cap, ms):
            self._max_systems = ms
            check(self._fn("set_params")(self._h, *self._params))
            if self._precision:
                check(self._fn("set_precision")(self._h, self._precision))
            self._layout_sent = False
        if not self._layout_sent:
            check(self._hctx._lib.nbody_hip_hermite_batch_set_layout(self._h, self._offsets.ctypes.data,
                                                                     self._offsets.size - 1))
            self._layout_sent = True
            for key, send in self._FEATURES.items():  # (set_layout dropped the handle's configuration)
                if getattr(self, key) is not None:
                    getattr(self, send)()
        return self._h

    @staticmethod
    def _ptr(a):
        return None if a is None else a.ctypes.data

    def _send_events(self):
        radii, limits, flags = self._events
        check(self._hctx._lib.nbody_hip_hermite_batch_set_events(self._h, self._ptr(radii), self._ptr(limits), flags))

    def _send_outcomes(self):
        radii, flags = self._outcomes
        check(self._hctx._lib.nbody_hip_batch_outcomes_set(self._h, self._ptr(radii), flags))

    def _send_hierarchy(self):
        radii, kappa, flags = self._hierarchy
        check(self._hctx._lib.nbody_hip_batch_hierarchy_set(self._h, self._ptr(radii), kappa, flags))

    def _send_mergers(self):
        check(self._hctx._lib.nbody_hip_batch_mergers_set(self._h, self._mergers))

    def _drop_features(self):
        for key in self._FEATURES:
            setattr(self, key, None)

    def _configure(self, key, value, off=False):
        """Keeps `value` as the configuration `key` and sends it to a handle that has the layout.  Where the library
        refuses or fails, the handle keeps what it had, and so does this.  off: the value turns the feature off, and
        nothing is kept of it."""
        before = getattr(self, key)
        setattr(self, key, value)
        try:
            if self._h is not None and self._layout_sent:
                getattr(self, self._FEATURES[key])()
        except BaseException:
            setattr(self, key, before)
            raise
        if off:
            setattr(self, key, None)

    def _system_radii(self, value, arg, noun):
        """a scalar or an array of B non-negative finite values as float32 [B], one per system; None stays None"""
        if self._offsets is None:
            raise StateException("the ensemble has no layout: call setLayout first")
        if value is None:
            return None
        systems = self._offsets.size - 1
        r = np.asarray(value)
        if r.dtype.kind not in "fiu":
            raise ValidationException(f"{arg} must be real numbers, got dtype {r.dtype}")
        if r.ndim == 0:
            r = np.full(systems, r)
        if r.shape != (systems,):
            raise ValidationException(f"{arg} must be a scalar or an array of {systems} values, one per system, got shape "
                                      f"{r.shape}")
        r = np.ascontiguousarray(r, np.float32)
        bad = np.flatnonzero(~(np.isfinite(r) & (r >= 0)))
        if bad.size:
            raise ValidationException(f"the {noun} radius of system {int(bad[0])} must be non-negative and finite, got "
                                      f"{float(r[bad[0]])}")
        return r

    def setLayout(self, offsets):
        """offsets: B + 1 integers, offsets[0] = 0, strictly ascending, every size in [1, 4096] (ic.concat returns
        them).  A new layout unprimes the ensemble."""
        self._offsets = self._check_offsets(offsets)
        self._layout_sent = False
        self._drop_features()  # (the radii were per body or per system of the old layout)
        if self._h is not None and int(self._offsets.max()) <= self._capacity and self._offsets.size - 1 <= self._max_systems:
            check(self._hctx._lib.nbody_hip_hermite_batch_set_layout(self._h, self._offsets.ctypes.data,
                                                                     self._offsets.size - 1))
            self._layout_sent = True

    def prime(self, d_particles: ParticleData, force_calc, dt_max):
        """(a, j) of every system at the current state and the start levels: overwrites acc_*.  dt_max: a scalar for
        all systems or an array of B values."""
        fc = self._direct(force_calc, "prime")
        if self._offsets is None:
            raise StateException("the ensemble has no layout: call setLayout first")
        systems = self._offsets.size - 1
        dt = np.asarray(dt_max, np.float32)
        if dt.ndim == 0:
            dt = np.full(systems, dt, np.float32)
        if dt.shape != (systems,):
            raise ValidationException(f"dt_max must be a scalar or an array of {systems} values, got shape {dt.shape}")
        dt = np.ascontiguousarray(dt)
        h = self._handle(d_particles, fc)
        s = d_particles.struct()
        check(self._hctx._lib.nbody_hip_hermite_batch_prime(h, C.byref(s), fc.G_, fc.softening_eps_, dt.ctypes.data))
        self._count = d_particles.count

    def advance(self, d_particles: ParticleData, macro_steps: int = 1):
        """Every system to its next `macro_steps` macro boundaries in one launch (asynchronous); macro_steps <= 0 does
        nothing.  StateException on an unprimed ensemble."""
        if macro_steps <= 0:
            return
        self._require_primed()
        s = d_particles.struct()
        check(self._hctx._lib.nbody_hip_hermite_batch_advance(self._h, C.byref(s), int(macro_steps)))

    def setEvents(self, radii=None, max_macro_steps=None, track_closest: bool = False, stop_on_contact: bool = False):
        """Per-system stopping conditions and encounter records (nbody_hip_hermite_batch_set_events; include/nbody_hip.h,
        "ensemble EVENTS").  radii: one non-negative finite value per body of the ensemble, or None; max_macro_steps: one
        budget per system in macro steps since the priming (0: none), a scalar for all, or None; track_closest: keep the
        closest approach; stop_on_contact: a system whose first contact has been recorded completes its macro step and
        stops (needs radii).  After setLayout; a new layout drops it.  setEvents() with nothing returns the ensemble to
        the plain kernel.  A recorded advance keeps the kernel form it recorded: record again after changing this."""
        if self._offsets is None:
            raise StateException("the ensemble has no layout: call setLayout first")
        total, systems = int(self._offsets[-1]), self._offsets.size - 1
        r = lim = None
        if radii is not None:
            r = np.asarray(radii)
            if r.dtype.kind not in "fiu":
                raise ValidationException(f"radii must be real numbers, got dtype {r.dtype}")
            if r.shape != (total,):
                raise ValidationException(f"radii must be an array of {total} values, one per body, got shape {r.shape}")
            r = np.ascontiguousarray(r, np.float32)
            bad = np.flatnonzero(~(np.isfinite(r) & (r >= 0)))
            if bad.size:
                raise ValidationException(f"the radius of body {int(bad[0])} must be non-negative and finite, got "
                                          f"{float(r[bad[0]])}")
        if max_macro_steps is not None:
            lim = np.asarray(max_macro_steps)
            if lim.dtype.kind not in "iu":
                raise ValidationException(f"max_macro_steps must be integers, got dtype {lim.dtype}")
            if lim.ndim == 0:
                lim = np.full(systems, lim)
            if lim.shape != (systems,):
                raise ValidationException(f"max_macro_steps must be a scalar or an array of {systems} values, got shape "
                                          f"{lim.shape}")
            if lim.dtype.kind == "i" and (lim < 0).any():
                raise ValidationException("max_macro_steps must not be negative (0: no limit)")
            lim = np.ascontiguousarray(lim, np.uint64)
        if stop_on_contact and r is None:
            raise ValidationException("stop_on_contact needs radii: without them no pair is ever in contact")
        flags = (_lib.BATCH_EVENTS_TRACK_CLOSEST if track_closest else 0) | \
                (_lib.BATCH_EVENTS_STOP_ON_CONTACT if stop_on_contact else 0)
        self._configure("_events", (r, lim, flags))

    def events(self) -> np.ndarray:
        """The records of all systems as a numpy structured array (BATCH_EVENT_DTYPE), one row per system: stopped
        (0 running, 1 contact, 2 budget, 3 escape: EnsembleOutcomes, 4 resolved: EnsembleHierarchy), macro_steps_done, closest_{d2, i, j, macro, tick}, contact_{d2, i, j, macro,
        tick}; "none" is d2 = +inf with indices BATCH_EVENT_NONE.  Blocks.  StateException on an unprimed ensemble."""
        self._require_primed(self._offsets is not None)
        out = np.zeros(self._offsets.size - 1, BATCH_EVENT_DTYPE)
        check(self._hctx._lib.nbody_hip_hermite_batch_events(self._h, out.ctypes.data, out.size))
        return out

    def running(self) -> int:
        """The number of systems that have neither stopped nor met a schedule error: `while ens.running(): ens.advance(d, k)`.
        Blocks.  StateException on an unprimed ensemble."""
        self._require_primed()
        n = C.c_size_t(0)
        check(self._hctx._lib.nbody_hip_hermite_batch_running(self._h, C.byref(n)))
        return int(n.value)

    def diagnostics_into(self, d_particles: ParticleData, out: torch.Tensor):
        """nbody_hip_hermite_batch_diagnostics, asynchronous: the struct of every system of the layout into `out`
        (system_diag_tensor(B, device)), from the full state (the residuals in "extended" mode) with the primed G and
        eps.  Allocates nothing and reads nothing back: it can be recorded into a step graph, after advance() for
        instance.  StateException on an unprimed ensemble."""
        self._require_primed(self._offsets is not None)
        _diag_out(out, self._offsets.size - 1, d_particles.pos_x.device)
        s = d_particles.struct()
        check(self._hctx._lib.nbody_hip_hermite_batch_diagnostics(self._h, C.byref(s), out.data_ptr()))
        return out

    def diagnostics(self, d_particles: ParticleData) -> np.ndarray:
        """Per-system fp64 diagnostics as a numpy structured array (SYSTEM_DIAG_DTYPE), one row per system: energies,
        momenta, the closest and the most bound pair (systems_diagnostics).  Blocks for the copy."""
        self._require_primed(self._offsets is not None)
        out = system_diag_tensor(self._offsets.size - 1, d_particles.pos_x.device)
        self.diagnostics_into(d_particles, out)
        self._hctx.synchronize()
        return system_diag_array(out)

    def info(self, system=None) -> dict:
        """The counters of system `system` since the last priming, or (None) their sums over the systems."""
        return self._info(-1 if system is None else int(system))

    def close(self):
        super().close()
        self._max_systems = 0


class _EnsembleCompanion:
    """what the companions of a BlockHermiteEnsemble share: they hold the ensemble, configure its handle and read from it"""

    def __init__(self, ensemble: BlockHermiteEnsemble):
        if not isinstance(ensemble, BlockHermiteEnsemble):
            raise ValidationException(f"{type(self).__name__} needs a BlockHermiteEnsemble, got {type(ensemble).__name__}")
        self._ens = ensemble


class EnsembleOutcomes(_EnsembleCompanion):
    """Per-system escape detection and stop-on-escape of a BlockHermiteEnsemble (nbody_hip_batch_outcomes_*;
    include/nbody_hip.h, "ensemble OUTCOMES").  A companion of the ensemble, not a part of it: it configures the
    ensemble's handle and reads the outcome records; the ensemble's events()["stopped"] (BATCH_STOPPED_ESCAPE) and
    running() reflect a stop.  After every completed macro step a system with an escape radius tests each body against
    the centre of mass of all the rest: beyond the radius, moving outward and unbound is an escape.  Single-body escapers
    only: choose the radius well outside any bound structure of interest."""

    def set(self, escape_radius=None, stop_on_escape: bool = False):
        """escape_radius: a scalar for all systems or an array of B values, non-negative and finite, 0: no test for that
        system; None turns the outcomes off.  stop_on_escape: a system with a first escape stops (needs a radius > 0).
        After setLayout; a new layout drops it.  A recorded advance keeps the kernel form it recorded: run one eager
        advance and record again after changing this."""
        r = self._ens._system_radii(escape_radius, "escape_radius", "escape")
        if stop_on_escape and (r is None or not (r > 0).any()):
            raise ValidationException("stop_on_escape needs an escape radius > 0: without one no body ever escapes")
        self._ens._configure("_outcomes", (r, _lib.BATCH_OUTCOMES_STOP_ON_ESCAPE if stop_on_escape else 0), off=r is None)

    def records(self) -> np.ndarray:
        """The outcome records of all systems as a numpy structured array (BATCH_OUTCOME_DTYPE), one row per system:
        escaped (the count at the boundary of the first escape, 0: none), escaper (the lowest escaping index), macro, r,
        vr, energy, rest_mass.  Blocks.  StateException on an unprimed ensemble."""
        ens = self._ens
        ens._require_primed(ens._offsets is not None)
        out = np.zeros(ens._offsets.size - 1, BATCH_OUTCOME_DTYPE)
        check(ens._hctx._lib.nbody_hip_batch_outcomes_get(ens._h, out.ctypes.data, out.size))
        return out


class EnsembleMergers(_EnsembleCompanion):
    """Sticky-sphere mergers of a BlockHermiteEnsemble, applied between launches (nbody_hip_batch_mergers_*;
    include/nbody_hip.h, "ensemble MERGERS").  A companion of the ensemble, like EnsembleOutcomes.  The ensemble needs
    setEvents(radii, stop_on_contact=True): a system whose first contact is on record stops at the end of that macro
    step; apply() then merges the recorded pair of every such system on the device (mass and momentum conserved, the
    volume rule for the radius), shrinks the system by one body in place, primes it again alone and lets it run on.  One
    merger per system per apply(); the indices of event, outcome and hierarchy records are slots, ids() translates them
    to the indices the bodies had at the priming.  The merger is applied at the macro boundary, not at the contact tick.
    A priming after mergers needs the radii set again (setEvents): those of merged systems have changed."""

    def set(self, enabled: bool = True):
        """Turns the mergers on or off.  After setLayout; a new layout drops it."""
        ens = self._ens
        if ens._offsets is None:
            raise StateException("the ensemble has no layout: call setLayout first")
        if not isinstance(enabled, (bool, np.bool_)):
            raise ValidationException(f"enabled must be True or False, got {enabled!r}")
        ens._configure("_mergers", _lib.BATCH_MERGERS_ON if enabled else 0, off=not enabled)

    def apply(self, d_particles: ParticleData):
        """One pass (asynchronous): every system that stopped on contact merges its recorded pair and runs on.  After one
        eager call since the priming it can be recorded into a step graph.  StateException on an unprimed ensemble,
        without set(), or without setEvents(radii, stop_on_contact=True)."""
        ens = self._ens
        ens._require_primed()
        if ens._mergers is None:
            raise StateException("the ensemble's mergers are not configured: call set() first")
        if ens._events is None or ens._events[0] is None or not (ens._events[2] & _lib.BATCH_EVENTS_STOP_ON_CONTACT):
            raise StateException("mergers need setEvents(radii, stop_on_contact=True): without them no system ever stops "
                                 "on a contact")
        s = d_particles.struct()
        check(ens._hctx._lib.nbody_hip_batch_mergers_apply(ens._h, C.byref(s)))

    def run(self, d_particles: ParticleData, macro_steps: int, every: int = 1):
        """advance(every); apply() repeated until macro_steps macro steps have been asked for (the last advance is
        shorter when every does not divide macro_steps).  Asynchronous."""
        macro_steps, every = int(macro_steps), int(every)
        if every < 1:
            raise ValidationException(f"every must be at least 1, got {every}")
        done = 0
        while done < macro_steps:
            k = min(every, macro_steps - done)
            self._ens.advance(d_particles, k)
            self.apply(d_particles)
            done += k

    def _get(self, log: bool, ids: bool):
        ens = self._ens
        ens._require_primed(ens._offsets is not None)
        systems, total = ens._offsets.size - 1, int(ens._offsets[-1])
        state = np.zeros(systems, BATCH_MERGER_STATE_DTYPE)
        entries = np.zeros(total, BATCH_MERGER_ENTRY_DTYPE) if log else None
        idv = np.zeros(total, np.uint32) if ids else None
        check(ens._hctx._lib.nbody_hip_batch_mergers_get(ens._h, state.ctypes.data, systems,
                                                         None if entries is None else entries.ctypes.data,
                                                         None if idv is None else idv.ctypes.data, total))
        return state, entries, idv

    def records(self) -> np.ndarray:
        """The merger state of all systems (BATCH_MERGER_STATE_DTYPE), one row per system: n_live, n_mergers, flags
        (BATCH_MERGER_BAD_RECORD).  Blocks.  StateException on an unprimed ensemble."""
        return self._get(False, False)[0]

    def log(self) -> np.ndarray:
        """The log entries of all systems in system order, each system's in the order they were made
        (BATCH_MERGER_DTYPE: a system column, then the fields of nbody_hip_batch_merger_t).  Blocks."""
        state, entries, _ = self._get(True, False)
        first = self._ens._offsets[:-1].astype(np.int64)
        count = state["n_mergers"].astype(np.int64)
        system = np.repeat(np.arange(count.size), count)
        within = np.arange(int(count.sum())) - np.repeat(np.cumsum(count) - count, count)
        out = np.zeros(system.size, BATCH_MERGER_DTYPE)
        out["system"] = system
        picked = entries[first[system] + within]
        for name in BATCH_MERGER_ENTRY_DTYPE.names:
            out[name] = picked[name]
        return out

    def ids(self) -> np.ndarray:
        """Per body of the ensemble (uint32): the system-local index the body in that slot had at the priming;
        BATCH_EVENT_NONE in a dead slot.  Blocks."""
        return self._get(False, True)[2]

    def alive(self) -> np.ndarray:
        """A boolean mask over the ensemble's bodies: the slots below their system's live count.  Blocks."""
        state = self._get(False, False)[0]
        off = self._ens._offsets.astype(np.int64)
        sizes = np.diff(off)
        local = np.arange(int(off[-1])) - np.repeat(off[:-1], sizes)
        return local < np.repeat(state["n_live"].astype(np.int64), sizes)


class EnsembleHierarchy(_EnsembleCompanion):
    """Per-system decomposition into nested bound pairs and stop-when-resolved of a BlockHermiteEnsemble
    (nbody_hip_batch_hierarchy_*; include/nbody_hip.h, "ensemble HIERARCHIES").  A companion of the ensemble, like
    EnsembleOutcomes: it configures the ensemble's handle and reads the records and node tables; the ensemble's
    events()["stopped"] (BATCH_STOPPED_RESOLVED) and running() reflect a stop.  After every completed macro step a system
    of 2 to 64 bodies with a separation radius is reduced to a forest of bound pairs; it is resolved when the forest has
    two or more pieces that are mutually unbound, receding, farther apart than the radius and isolated."""

    def set(self, separation_radius=None, isolation: float = 0.0, stop_on_resolved: bool = False):
        """separation_radius: a scalar for all systems or an array of B values, non-negative and finite, 0: no
        examination for that system (required for a system of more than 64 bodies); None turns the hierarchies off.
        isolation: kappa, every two pieces must be farther apart than kappa times the sum of their apocentres (0: off).
        stop_on_resolved: a resolved system stops (needs a radius > 0).  After setLayout; a new layout drops it.  A
        recorded advance keeps the kernel form it recorded: run one eager advance and record again after changing this."""
        ens = self._ens
        r = ens._system_radii(separation_radius, "separation_radius", "separation")
        if r is not None:
            sizes = np.diff(ens._offsets.astype(np.int64))
            big = np.flatnonzero((r > 0) & (sizes > _lib.BATCH_HIERARCHY_MAX))
            if big.size:
                raise ValidationException(f"system {int(big[0])} has {int(sizes[big[0]])} bodies: a hierarchy is examined in "
                                          f"systems of at most {_lib.BATCH_HIERARCHY_MAX} (its separation radius must be 0, "
                                          f"got {float(r[big[0]])})")
        kappa = np.float32(isolation)
        if not (np.isfinite(kappa) and kappa >= 0):
            raise ValidationException(f"the isolation factor must be non-negative and finite, got {float(kappa)}")
        if stop_on_resolved and (r is None or not (r > 0).any()):
            raise ValidationException("stop_on_resolved needs a separation radius > 0: without one no system is ever examined")
        ens._configure("_hierarchy", (r, float(kappa) if r is not None else 0.0,
                                      _lib.BATCH_HIERARCHY_STOP_ON_RESOLVED if stop_on_resolved else 0), off=r is None)

    def _read(self, call):
        ens = self._ens
        rec = np.zeros(ens._offsets.size - 1, BATCH_HIERARCHY_DTYPE)
        nodes = np.zeros(2 * int(ens._offsets[-1]), BATCH_NODE_DTYPE)
        call(rec, nodes)
        return rec, nodes

    def records(self) -> np.ndarray:
        """The hierarchy records of all systems as a numpy structured array (BATCH_HIERARCHY_DTYPE), one row per system:
        resolved, top_count, macro, node_count, largest, min_sep, min_p, min_q.  Blocks.  StateException on an unprimed
        ensemble."""
        ens = self._ens
        ens._require_primed(ens._offsets is not None)
        out = np.zeros(ens._offsets.size - 1, BATCH_HIERARCHY_DTYPE)
        check(ens._hctx._lib.nbody_hip_batch_hierarchy_get(ens._h, out.ctypes.data, out.size, None, 0))
        return out

    def nodes(self, system=None) -> np.ndarray:
        """The node table (BATCH_NODE_DTYPE) of one system, its 2 n slots, or (None) of all systems back to back: system s
        has the slots [2 offsets[s], 2 offsets[s + 1]).  Blocks.  StateException on an unprimed ensemble."""
        ens = self._ens
        ens._require_primed(ens._offsets is not None)
        lib = ens._hctx._lib
        _, nodes = self._read(lambda rec, nodes: check(lib.nbody_hip_batch_hierarchy_get(
            ens._h, rec.ctypes.data, rec.size, nodes.ctypes.data, nodes.size)))
        return nodes if system is None else self._slice(nodes, system)

    def _slice(self, nodes, system):
        off = self._ens._offsets
        s = int(system)
        if not 0 <= s < off.size - 1:
            raise ValidationException(f"system must be in [0, {off.size - 1}), got {s}")
        return nodes[2 * int(off[s]):2 * int(off[s + 1])]

    def snapshot(self, d_particles: ParticleData):
        """(records, nodes) of the state as it is now, of every system of 2 to 64 bodies, stopped ones included, by a
        kernel of its own: the run's own records are not touched.  Blocks.  StateException on an unprimed ensemble."""
        ens = self._ens
        ens._require_primed(ens._offsets is not None)
        lib, s = ens._hctx._lib, d_particles.struct()
        return self._read(lambda rec, nodes: check(lib.nbody_hip_batch_hierarchy_snapshot(
            ens._h, C.byref(s), rec.ctypes.data, rec.size, nodes.ctypes.data, nodes.size)))

    def describe(self, system, nodes=None) -> str:
        """hierarchy_string of one system: of its slots in `nodes` (all systems' slots, as nodes() or snapshot() return
        them), or of the run's own table."""
        table = self.nodes(system) if nodes is None else self._slice(nodes, system)
        return hierarchy_string(table, table.shape[0] // 2)


# ---- packed (native) entry points ------------------------------------------------------------

def pack_posm(ctx: Context, x, y, z, m) -> torch.Tensor:
    n = x.numel()
    out = torch.empty((n, 4), dtype=torch.float32, device=x.device)
    check(ctx._lib.nbody_hip_pack_posm(ctx.handle, x.data_ptr(), y.data_ptr(), z.data_ptr(),
                                       m.data_ptr(), n, out.data_ptr()))
    return out


def direct_forces_packed(ctx: Context, targets: torch.Tensor, sources: torch.Tensor, G: float,
                         eps2: float, out: torch.Tensor | None = None, accumulate: bool = False):
    """targets [nt,4], sources [ns,4] float32 contiguous on the device -> acc [nt,4]."""
    assert targets.dtype == torch.float32 and sources.dtype == torch.float32
    assert targets.is_contiguous() and sources.is_contiguous()
    assert targets.dim() == 2 and targets.shape[1] == 4 and sources.dim() == 2 and sources.shape[1] == 4
    nt, ns = targets.shape[0], sources.shape[0]
    if out is None:
        assert not accumulate
        out = torch.empty((nt, 4), dtype=torch.float32, device=targets.device)
    assert out.is_contiguous() and out.shape == (nt, 4)
    check(ctx._lib.nbody_hip_direct_forces_packed(ctx.handle, targets.data_ptr(), nt,
                                                  sources.data_ptr(), ns, out.data_ptr(), G, eps2,
                                                  1 if accumulate else 0))
    return out


def direct_forces_pair_packed(ctx: Context, a: torch.Tensor, b: torch.Tensor, G: float, eps2: float,
                              acc_a: torch.Tensor, acc_b: torch.Tensor, accumulate_a: bool = False,
                              accumulate_b: bool = False):
    """Two disjoint body sets, each a x b pair evaluated once: acc_a (+)= forces on a from b,
    acc_b (+)= forces on b from a (the reactions)."""
    for t in (a, b, acc_a, acc_b):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == 4
    assert acc_a.shape == a.shape and acc_b.shape == b.shape
    check(ctx._lib.nbody_hip_direct_forces_pair_packed(
        ctx.handle, a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], acc_a.data_ptr(),
        1 if accumulate_a else 0, acc_b.data_ptr(), 1 if accumulate_b else 0, G, eps2))


def time_direct_packed(ctx: Context, targets, sources, G, eps2, iters: int, out=None) -> float:
    nt, ns = targets.shape[0], sources.shape[0]
    if out is None:
        out = torch.empty((nt, 4), dtype=torch.float32, device=targets.device)
    ms = C.c_float()
    check(ctx._lib.nbody_hip_time_direct_packed(ctx.handle, targets.data_ptr(), nt,
                                                sources.data_ptr(), ns, out.data_ptr(), G, eps2,
                                                iters, C.byref(ms)))
    return ms.value


def direct_acc_jerk(ctx: Context, d_particles: ParticleData, G: float, eps: float, write_acc: bool = False):
    """Direct acceleration and jerk at the bodies (nbody_hip_direct_acc_jerk): -> (acc [N, 4], jerk [N, 4]) device
    tensors {x, y, z, 0}; acc_* are not written.  With write_acc=True the accelerations go to acc_* instead and the
    first element returned is None.  Takes eps (not eps^2)."""
    n = d_particles.count
    dev = d_particles.pos_x.device
    jerk = torch.empty((n, 4), dtype=torch.float32, device=dev)
    acc = None if write_acc else torch.empty((n, 4), dtype=torch.float32, device=dev)
    s = d_particles.struct()
    check(ctx._lib.nbody_hip_direct_acc_jerk(ctx.handle, C.byref(s), G, eps, None if acc is None else acc.data_ptr(),
                                             jerk.data_ptr()))
    return acc, jerk


def direct_acc_jerk_ext(ctx: Context, d_particles: ParticleData, pos_lo: torch.Tensor, G: float, eps: float,
                        write_acc: bool = False):
    """direct_acc_jerk at the double-single positions pos + pos_lo (nbody_hip_direct_acc_jerk_ext): pos_lo an [N, 4]
    float32 device tensor {lx, ly, lz, 0}.  -> (acc [N, 4], jerk [N, 4])."""
    n = d_particles.count
    dev = d_particles.pos_x.device
    if pos_lo.dtype != torch.float32 or tuple(pos_lo.shape) != (n, 4) or not pos_lo.is_contiguous():
        raise ValidationException(f"pos_lo must be a contiguous float32 tensor of shape ({n}, 4)")
    if pos_lo.device != dev:
        raise ValidationException("pos_lo must live on the device of the particle data")
    jerk = torch.empty((n, 4), dtype=torch.float32, device=dev)
    acc = None if write_acc else torch.empty((n, 4), dtype=torch.float32, device=dev)
    s = d_particles.struct()
    check(ctx._lib.nbody_hip_direct_acc_jerk_ext(ctx.handle, C.byref(s), pos_lo.data_ptr(), G, eps,
                                                 None if acc is None else acc.data_ptr(), jerk.data_ptr()))
    return acc, jerk
