"""ParticleSystem facade, SimulationState and the `.nbody` checkpoint (host side, Python).

  ParticleSystem    include/nbody/particle_system.hpp:139-393, src/core/particle_system.cpp:40-318
  SimulationState   include/nbody/simulation_state.hpp, src/utils/simulation_state.cpp:7-39
  Serializer        include/nbody/serialization.hpp:36-137, src/utils/serialization.cpp:9-135
                    (56-byte header {magic 0x4E424F44, version 1, u64 count, time, dt, G, eps,
                    method, reserved[4], pad} + pos_x,y,z, vel_x,y,z, mass as raw fp32)

Orchestration only: every force / integration / energy call goes through the C ABI via api.py.
The C++ counterpart is the reference's own particle_system.cpp linked against libnbody_facade.so
(oracle/Makefile.ref).
"""
from __future__ import annotations

import io
import struct
from dataclasses import dataclass, field

import numpy as np
import torch

from ._lib import StateException, ValidationException
from .api import (BarnesHutCalculator, DiskDistParams, ForceMethod, HermiteIntegrator, BlockHermiteIntegrator, InitDistribution, Integrator,
                  ParticleData, ParticleDataManager, ParticleInitializer, SimulationConfig, SpatialHashCalculator, SpatialHashGrid, GroupCatalogue, NeighbourLists, HopCatalogue, _hop_on_lists, density_centre, groups_radial_profile,
                  SphericalDistParams, UniformDistParams,
                  createForceCalculator, validateSimulationConfig, validateSoftening,
                  validateTheta, validateTimeStep, _finite, STATE_PRECISIONS, BLOCK_SCHEDULINGS)

NBODY_MAGIC = 0x4E424F44
NBODY_VERSION = 1
MAX_PARTICLE_COUNT = 100_000_000
_HEADER = struct.Struct("<IIQffffI4I4x")  # 56 bytes, natural alignment of the C struct
assert _HEADER.size == 56
_ARRAYS = ("pos_x", "pos_y", "pos_z", "vel_x", "vel_y", "vel_z", "mass")
INTEGRATION_SCHEMES = ("velocity-verlet", "hermite4", "hermite4-block")
HERMITE_SCHEMES = ("hermite4", "hermite4-block")  # Direct-only


def _f32(n=0):
    return np.zeros(n, dtype=np.float32)


@dataclass
class SimulationState:
    pos_x: np.ndarray = field(default_factory=_f32)
    pos_y: np.ndarray = field(default_factory=_f32)
    pos_z: np.ndarray = field(default_factory=_f32)
    vel_x: np.ndarray = field(default_factory=_f32)
    vel_y: np.ndarray = field(default_factory=_f32)
    vel_z: np.ndarray = field(default_factory=_f32)
    mass: np.ndarray = field(default_factory=_f32)
    particle_count: int = 0
    simulation_time: float = 0.0
    dt: float = 0.0
    G: float = 0.0
    softening: float = 0.0
    force_method: ForceMethod = ForceMethod.DIRECT_N2

    def __eq__(self, other):  # simulation_state.cpp:7-39: scalars exact, arrays within 1e-6
        if not isinstance(other, SimulationState):
            return NotImplemented
        if (self.particle_count != other.particle_count or self.force_method != other.force_method):
            return False
        for k in ("simulation_time", "dt", "G", "softening"):
            if abs(np.float32(getattr(self, k)) - np.float32(getattr(other, k))) > 1e-6:
                return False
        for k in _ARRAYS:
            a, b = getattr(self, k), getattr(other, k)
            if a.shape != b.shape or np.any(np.abs(a - b) > 1e-6):
                return False
        return True


class Serializer:
    @staticmethod
    def save(target, state: SimulationState):
        if isinstance(target, (str, bytes)):
            try:
                with open(target, "wb") as f:
                    Serializer.save(f, state)
            except OSError as e:
                raise RuntimeError(f"Failed to open file for writing: {target}") from e
            return
        target.write(_HEADER.pack(NBODY_MAGIC, NBODY_VERSION, int(state.particle_count),
                                  float(np.float32(state.simulation_time)), float(np.float32(state.dt)),
                                  float(np.float32(state.G)), float(np.float32(state.softening)),
                                  int(state.force_method), 0, 0, 0, 0))
        for k in _ARRAYS:
            target.write(np.ascontiguousarray(getattr(state, k), dtype="<f4").tobytes())

    @staticmethod
    def readHeader(stream):
        raw = stream.read(_HEADER.size)
        if len(raw) != _HEADER.size:
            raise RuntimeError("Failed to read file header: file may be truncated or corrupted")
        magic, version, count, t, dt, G, eps, method, *_ = _HEADER.unpack(raw)
        if magic != NBODY_MAGIC:
            raise RuntimeError("Invalid file format: wrong magic number")
        if version != NBODY_VERSION:
            raise RuntimeError("Unsupported file version")
        return dict(particle_count=count, simulation_time=t, dt=dt, G=G, softening=eps, force_method=method)

    @staticmethod
    def load(source) -> SimulationState:
        if isinstance(source, (str, bytes)):
            try:
                f = open(source, "rb")
            except OSError as e:
                raise RuntimeError(f"Failed to open file for reading: {source}") from e
            with f:
                return Serializer.load(f)
        h = Serializer.readHeader(source)
        n = h["particle_count"]
        if n > MAX_PARTICLE_COUNT:
            raise ValidationException(f"Particle count ({n}) exceeds maximum allowed ({MAX_PARTICLE_COUNT})")
        st = SimulationState(particle_count=n, simulation_time=h["simulation_time"], dt=h["dt"], G=h["G"],
                             softening=h["softening"], force_method=ForceMethod(h["force_method"]))
        for k in _ARRAYS:
            raw = source.read(4 * n)
            if len(raw) != 4 * n:
                raise RuntimeError("Failed to read particle data: file may be truncated or corrupted")
            setattr(st, k, np.frombuffer(raw, dtype="<f4").astype(np.float32))
        return st

    @staticmethod
    def validateFile(filename) -> bool:
        try:
            with open(filename, "rb") as f:
                Serializer.readHeader(f)
            return True
        except (OSError, RuntimeError):
            return False


class ParticleSystem:
    """The user-facing facade of the reference (particle_system.hpp:139-393)."""

    def __init__(self):
        self.d_particles_ = ParticleData()
        self.h_particles_ = ParticleData()
        self.particle_count_ = 0
        self.force_calculator_ = None
        self.integrator_ = None
        self.dt_, self.G_, self.softening_ = 0.001, 1.0, 0.1
        self.simulation_time_ = 0.0
        self.force_method_ = ForceMethod.DIRECT_N2
        self.is_paused_ = False
        self.is_initialized_ = False
        self.config_ = SimulationConfig()
        self.bh_multipole_order_ = 1  # not in SimulationConfig (the reference's 48-byte POD)
        self.integration_scheme_ = "velocity-verlet"  # (nor is this; not stored in a checkpoint either)
        self.hermite_ = None
        self.hermite_block_ = None
        self.hermite_precision_ = "fp32"  # state precision of the two Hermite schemes (not in the checkpoint either)
        self.hermite_block_scheduling_ = "host"  # where "hermite4-block" schedules its block steps (likewise)
        self.group_grid_ = None  # the private grid of findGroups (created at its first call)
        self.neighbour_grid_ = None  # the private grid of localDensity / densityCentre (created at their first call)

    # -- memory ------------------------------------------------------------------------------
    def _allocate(self, count):
        self.particle_count_ = count
        ParticleDataManager.allocateDevice(self.d_particles_, count)
        ParticleDataManager.allocateHost(self.h_particles_, count)

    def _free(self):
        if self.is_initialized_:
            ParticleDataManager.freeDevice(self.d_particles_)
            ParticleDataManager.freeHost(self.h_particles_)
            self.is_initialized_ = False

    def _invalidate_hermite(self):
        """state or parameters changed behind the Hermite integrator: its next step primes (a, j) again"""
        if self.hermite_ is not None:
            self.hermite_.invalidate()
        if self.hermite_block_ is not None:
            self.hermite_block_.invalidate()

    def _reprime_hermite(self):
        """G or eps changed: (a, j) must be primed again, the state did not change.  In fp32 mode that is an
        invalidation; in extended mode the step primes again by itself for another G or eps, which keeps the residuals
        (an invalidation would zero them)"""
        if self.hermite_precision_ == "fp32":
            self._invalidate_hermite()

    def _check_scheme(self, scheme, method):
        if scheme in HERMITE_SCHEMES and method != ForceMethod.DIRECT_N2:
            raise ValidationException(f"integration scheme '{scheme}' is Direct-only (the tree and the grid have no "
                                      f"jerk): the force method is {ForceMethod(method).name}")

    def _create_calculator(self):
        self.force_calculator_ = createForceCalculator(self.force_method_, self.config_)
        self.force_calculator_.setGravitationalConstant(self.G_)
        self.force_calculator_.setSofteningParameter(self.softening_)
        if isinstance(self.force_calculator_, BarnesHutCalculator):
            self.force_calculator_.setMultipoleOrder(self.bh_multipole_order_)

    # -- lifecycle (particle_system.cpp:40-127) ------------------------------------------------
    def initialize(self, config: SimulationConfig, initial_conditions: dict | None = None):
        """`initial_conditions` (an ic.* dict) is an extension: the reference only knows its three
        built-in distributions (box +-10 / sphere R=10 / disk R=10,h=1,omega=0.5, :55-79)."""
        validateSimulationConfig(config)
        self._check_scheme(self.integration_scheme_, config.force_method)
        self._invalidate_hermite()
        self.config_ = SimulationConfig(**vars(config))
        self.dt_, self.G_, self.softening_ = config.dt, config.G, config.softening
        self.force_method_ = config.force_method
        self.is_paused_ = False
        self._free()
        n = config.particle_count
        self._allocate(n)
        if initial_conditions is None:
            # particle_system.cpp:53-79, default seed 42 (particle_data.hpp:38-57): the same bodies as the
            # reference's C++ ParticleSystem under libstdc++ (api.ParticleInitializer)
            if config.init_distribution == InitDistribution.UNIFORM:
                ParticleInitializer.initUniform(self.h_particles_, UniformDistParams((-10, -10, -10), (10, 10, 10)))
            elif config.init_distribution == InitDistribution.SPHERICAL:
                ParticleInitializer.initSpherical(self.h_particles_, SphericalDistParams((0, 0, 0), 10.0))
            else:
                ParticleInitializer.initDisk(self.h_particles_, DiskDistParams((0, 0, 0), 10.0, 1.0, rotation_speed=0.5))
        else:
            for k, v in initial_conditions.items():
                getattr(self.h_particles_, k)[:] = v
        ParticleDataManager.copyToDevice(self.d_particles_, self.h_particles_)
        self._create_calculator()
        self.integrator_ = Integrator(config.cuda_block_size)
        self.force_calculator_.computeForces(self.d_particles_)  # a(0), :88-91
        self.simulation_time_ = 0.0
        self.is_initialized_ = True

    def initializeWithDistribution(self, particle_count, dist):
        self.initialize(SimulationConfig(particle_count=particle_count, init_distribution=dist))

    def update(self, dt: float):
        if not self.is_initialized_ or self.is_paused_:
            return
        if self.integration_scheme_ == "hermite4":
            if self.hermite_ is None:
                self.hermite_ = HermiteIntegrator(self.config_.cuda_block_size)
                self.hermite_.setStatePrecision(self.hermite_precision_)
            self.hermite_.integrate(self.d_particles_, self.force_calculator_, dt)
        elif self.integration_scheme_ == "hermite4-block":  # dt is the macro step
            if self.hermite_block_ is None:
                self.hermite_block_ = BlockHermiteIntegrator(self.config_.cuda_block_size)
                self.hermite_block_.setStatePrecision(self.hermite_precision_)
                self.hermite_block_.setScheduling(self.hermite_block_scheduling_)
            self.hermite_block_.integrate(self.d_particles_, self.force_calculator_, dt)
        else:
            self.integrator_.integrate(self.d_particles_, self.force_calculator_, dt)
        self.simulation_time_ = float(np.float32(self.simulation_time_) + np.float32(dt))

    def pause(self):
        self.is_paused_ = True

    def resume(self):
        self.is_paused_ = False

    def isPaused(self):
        return self.is_paused_

    def reset(self):
        if self.is_initialized_:
            self.initialize(self.config_)

    # -- parameters (:137-207) -----------------------------------------------------------------
    def setForceMethod(self, method: ForceMethod):
        self._check_scheme(self.integration_scheme_, method)
        if self.force_method_ != method:
            self.force_method_ = method
            self.config_.force_method = method
            self._create_calculator()

    def setGravitationalConstant(self, G):
        if G <= 0 or not _finite(G):
            raise ValidationException("Gravitational constant must be positive and finite")
        self.G_ = self.config_.G = G
        self._reprime_hermite()
        if self.force_calculator_:
            self.force_calculator_.setGravitationalConstant(G)

    def setSofteningParameter(self, eps):
        validateSoftening(eps)
        self.softening_ = self.config_.softening = eps
        self._reprime_hermite()
        if self.force_calculator_:
            self.force_calculator_.setSofteningParameter(eps)

    def setTimeStep(self, dt):
        validateTimeStep(dt)
        self.dt_ = self.config_.dt = dt

    def setIntegrationScheme(self, scheme: str):
        """"velocity-verlet" (default, the reference's integrator), "hermite4" (HermiteIntegrator: fourth order) or
        "hermite4-block" (BlockHermiteIntegrator: the same scheme with individual block time steps, update(dt) is one
        macro step).  Both Hermite schemes are Direct only -- refused here with another force method, and setForceMethod
        refuses to leave Direct while one is selected.  update(dt) dispatches on it.  Not part of SimulationConfig or of the checkpoint."""
        if scheme not in INTEGRATION_SCHEMES:
            raise ValidationException(f"integration scheme must be one of {INTEGRATION_SCHEMES}, got {scheme!r}")
        self._check_scheme(scheme, self.force_method_)
        if scheme != self.integration_scheme_:
            self._invalidate_hermite()  # (velocity-verlet steps in between move the bodies behind it)
        self.integration_scheme_ = scheme

    def getIntegrationScheme(self) -> str:
        return self.integration_scheme_

    def setHermiteStatePrecision(self, precision: str):
        """"fp32" (default) or "extended": the state precision of the schemes "hermite4" and "hermite4-block"
        (HermiteIntegrator.setStatePrecision).  In extended mode the bodies' state is pos + pos_lo, vel + vel_lo with
        fp32 residuals kept by the integrator; pos_* / vel_* stay the fp32 roundings, and saveState writes those: a run
        continued from a checkpoint restarts from the ROUNDED state.  A switch re-primes and starts from the rounded
        state.  setGravitationalConstant, setSofteningParameter and setTimeStep keep the residuals; setState, loadState,
        reset, initialize and a switch of the scheme lose them.  Like the scheme, not part of SimulationConfig or of
        the checkpoint."""
        if not isinstance(precision, str) or precision not in STATE_PRECISIONS:
            raise ValidationException(f"state precision must be one of {STATE_PRECISIONS}, got {precision!r}")
        if precision != self.hermite_precision_:
            self._invalidate_hermite()
        self.hermite_precision_ = precision
        for integ in (self.hermite_, self.hermite_block_):
            if integ is not None:
                integ.setStatePrecision(precision)

    def getHermiteStatePrecision(self) -> str:
        return self.hermite_precision_

    def setHermiteBlockScheduling(self, scheduling: str):
        """"host" (default), "resident" or "auto": where the scheme "hermite4-block" schedules its block steps
        (BlockHermiteIntegrator.setScheduling).  With "resident" an update(dt) is one launch of one workgroup and does not
        wait for the device; it takes at most 4,096 bodies.  Every update() ends at a macro boundary, so a switch goes
        through at once.  Like the state precision, not part of SimulationConfig or of the checkpoint."""
        if not isinstance(scheduling, str) or scheduling not in BLOCK_SCHEDULINGS:
            raise ValidationException(f"block-step scheduling must be one of {BLOCK_SCHEDULINGS}, got {scheduling!r}")
        if self.hermite_block_ is not None:
            self.hermite_block_.setScheduling(scheduling)
        self.hermite_block_scheduling_ = scheduling

    def getHermiteBlockScheduling(self) -> str:
        return self.hermite_block_scheduling_

    def getExtendedState(self):
        """(X [N, 3], V [N, 3]) in fp64: pos + pos_lo and vel + vel_lo of the selected Hermite scheme in extended mode,
        else pos_* / vel_* widened."""
        if not self.is_initialized_:
            raise StateException("the particle system is not initialized")
        integ = {"hermite4": self.hermite_, "hermite4-block": self.hermite_block_}.get(self.integration_scheme_)
        if integ is None or self.hermite_precision_ == "fp32":
            return HermiteIntegrator().getExtendedState(self.d_particles_)
        return integ.getExtendedState(self.d_particles_)

    def setBarnesHutTheta(self, theta):
        validateTheta(theta)
        self.config_.barnes_hut_theta = theta
        if isinstance(self.force_calculator_, BarnesHutCalculator):
            self.force_calculator_.setTheta(theta)

    def setBarnesHutMultipoleOrder(self, order):
        """Multipole order of the Barnes-Hut tree (1 = monopoles, the default; 2 = monopoles + quadrupoles): kept
        across setForceMethod, reset and initialize; applies from the next update / computeMethodPotentialEnergy."""
        if int(order) not in (1, 2):
            raise ValidationException("multipole order must be 1 or 2")
        self.bh_multipole_order_ = int(order)
        if isinstance(self.force_calculator_, BarnesHutCalculator):
            self.force_calculator_.setMultipoleOrder(self.bh_multipole_order_)

    def getBarnesHutMultipoleOrder(self):
        return self.bh_multipole_order_

    def setSpatialHashCellSize(self, size):
        if size <= 0 or not _finite(size):
            raise ValidationException("Spatial hash cell size must be positive and finite")
        self.config_.spatial_hash_cell_size = size
        if isinstance(self.force_calculator_, SpatialHashCalculator):
            self.force_calculator_.setCellSize(size)

    def setSpatialHashCutoff(self, cutoff):
        if cutoff <= 0 or not _finite(cutoff):
            raise ValidationException("Spatial hash cutoff must be positive and finite")
        self.config_.spatial_hash_cutoff = cutoff
        if isinstance(self.force_calculator_, SpatialHashCalculator):
            self.force_calculator_.setCutoffRadius(cutoff)

    def getForceMethod(self):
        return self.force_method_

    def getGravitationalConstant(self):
        return self.G_

    def getSofteningParameter(self):
        return self.softening_

    def getTimeStep(self):
        return self.dt_

    def getSimulationTime(self):
        return self.simulation_time_

    def getParticleCount(self):
        return self.particle_count_

    def getDeviceData(self):
        return self.d_particles_

    def copyToHost(self, h_particles: ParticleData):
        ParticleDataManager.copyToHost(h_particles, self.d_particles_)

    # -- state (:213-302) ----------------------------------------------------------------------
    def getState(self) -> SimulationState:
        h = ParticleData()
        ParticleDataManager.allocateHost(h, self.particle_count_)
        ParticleDataManager.copyToHost(h, self.d_particles_)
        st = SimulationState(particle_count=self.particle_count_, simulation_time=self.simulation_time_,
                             dt=self.dt_, G=self.G_, softening=self.softening_,
                             force_method=self.force_method_)
        for k in _ARRAYS:
            setattr(st, k, getattr(h, k).copy())
        return st

    def setState(self, state: SimulationState):
        cfg = SimulationConfig(**vars(self.config_))
        cfg.particle_count, cfg.dt, cfg.G = state.particle_count, state.dt, state.G
        cfg.softening, cfg.force_method = state.softening, state.force_method
        validateSimulationConfig(cfg)
        self._check_scheme(self.integration_scheme_, state.force_method)
        self._invalidate_hermite()
        self._free()
        self._allocate(state.particle_count)
        for k in _ARRAYS:
            getattr(self.h_particles_, k)[:] = getattr(state, k)
        # accelerations are not part of the state: zeroed, then recomputed (:274-283)
        ParticleDataManager.copyToDevice(self.d_particles_, self.h_particles_)
        self.simulation_time_ = state.simulation_time
        self.dt_, self.G_, self.softening_ = state.dt, state.G, state.softening
        self.force_method_ = state.force_method
        self.config_ = cfg
        self._create_calculator()
        self.integrator_ = Integrator(cfg.cuda_block_size)
        self.force_calculator_.computeForces(self.d_particles_)
        self.is_paused_ = False
        self.is_initialized_ = True

    def saveState(self, filename):
        Serializer.save(filename, self.getState())

    def loadState(self, filename):
        self.setState(Serializer.load(filename))

    # -- energies (:304-318) -------------------------------------------------------------------
    def computeKineticEnergy(self) -> float:
        return self.integrator_.computeKineticEnergy(self.d_particles_) if self.integrator_ else 0.0

    def computePotentialEnergy(self) -> float:
        if not self.integrator_:
            return 0.0
        return self.integrator_.computePotentialEnergy(self.d_particles_, self.G_, self.softening_)

    def computeTotalEnergy(self) -> float:
        return float(np.float32(self.computeKineticEnergy()) + np.float32(self.computePotentialEnergy()))

    # -- the force method's own potential (extension: ForceCalculator.computePotential) ---------------------------
    def computeMethodPotentialEnergy(self) -> float:
        """PE = 1/2 sum m phi in the force method's model: Direct sum, the tree's interaction lists, or the hash's
        shifted truncated potential (the energy a hash run conserves)."""
        if not self.integrator_:
            return 0.0
        return self.force_calculator_.computePotential(self.d_particles_)

    def computeMethodTotalEnergy(self) -> float:
        """fp64 KE + computeMethodPotentialEnergy()."""
        if not self.integrator_:
            return 0.0
        return self.integrator_.computeKineticEnergyF64(self.d_particles_) + self.computeMethodPotentialEnergy()

    def getPotential(self) -> np.ndarray:
        """phi_i of the force method's model (float32, body order) as a host array."""
        if not self.integrator_:
            return np.zeros(0, np.float32)
        phi = torch.empty(self.particle_count_, dtype=torch.float32, device=self.d_particles_.pos_x.device)
        self.force_calculator_.computePotential(self.d_particles_, phi)
        return phi.cpu().numpy()

    def computeFieldAt(self, points, out=None) -> torch.Tensor:
        """{ax, ay, az, phi} of the force method's model at `points` (float32 device tensor [M, 3] or [M, 4]; a host
        array is uploaded) as an [M, 4] device tensor -- maps, tracers, rotation curves.  The bodies are not touched."""
        if not self.integrator_:
            raise ValidationException("the system is not initialised")
        if not isinstance(points, torch.Tensor):
            points = torch.as_tensor(np.ascontiguousarray(points, np.float32), device=self.d_particles_.pos_x.device)
        return self.force_calculator_.computeField(self.d_particles_, points, out)

    # -- friends-of-friends groups (extension: SpatialHashGrid.findGroups), whatever the force method -------------
    @staticmethod
    def groupCellSize(lo, hi, count: int, linking_length: float) -> float:
        """The cell of the private grid findGroups builds: linking_length * 2^k (fp32) with the smallest k >= 0 for which
        the box [lo, hi] of the bodies, padded and divided as the build does it, gives at most 16 * count + 4096 cells --
        the density rule of the grid's start array."""
        cell = ParticleSystem._cellWithinBudget(lo, hi, count, linking_length)
        if cell is None:
            raise ValidationException("linking length too small for the box of the bodies")
        return cell

    @staticmethod
    def _cellWithinBudget(lo, hi, count: int, start: float):
        """start * 2^k (fp32) with the smallest k >= 0 for which the box [lo, hi], padded and divided as the build does
        it, gives at most 16 * count + 4096 cells; None when 200 doublings do not get there."""
        f = np.float32
        lo = np.asarray(lo, f) - f(0.001)
        hi = np.asarray(hi, f) + f(0.001)
        cell = f(start)
        for _ in range(200):
            cells = 1
            for a in range(3):
                cells *= int(np.ceil(f(f(hi[a] - lo[a]) / cell))) + 1
            if cells <= 16 * count + 4096:
                return float(cell)
            cell = f(cell * f(2))
        return None

    @staticmethod
    def neighbourCellSize(lo, hi, count: int) -> float:
        """The default level-0 cell of localDensity / densityCentre: the finest cell of the ladder (longest padded side
        of the box) * 2^-k for which the box gives at most 16 * count + 4096 cells -- the rule of groupCellSize."""
        f = np.float32
        side = f((np.asarray(hi, f) + f(0.001) - (np.asarray(lo, f) - f(0.001))).max())
        return ParticleSystem._cellWithinBudget(lo, hi, count, float(f(side * f(2.0 ** -24))))

    def findGroups(self, linking_length: float, min_members: int = 1) -> GroupCatalogue:
        """Friends-of-friends groups of the bodies with linking length b, for every force method: a private grid of cell
        b * 2^k (groupCellSize) is built on the current positions; the force calculator's own structures are not
        touched.  Returns a GroupCatalogue (device tensors labels, offsets, members; sizes(); systems())."""
        if not self.integrator_:
            raise ValidationException("the system is not initialised")
        if not (linking_length > 0 and _finite(linking_length)):
            raise ValidationException("linking length must be positive and finite")
        d = self.d_particles_
        pos = torch.stack((d.pos_x, d.pos_y, d.pos_z))
        lo, hi = pos.min(dim=1).values.cpu().numpy(), pos.max(dim=1).values.cpu().numpy()
        cell = self.groupCellSize(lo, hi, d.count, linking_length)
        grid = self.group_grid_
        if grid is None or grid.max_particles_ != d.count:
            if grid is not None:
                grid.close()
            grid = self.group_grid_ = SpatialHashGrid(d.count, cell)
        grid.setCellSize(cell)
        grid.build(d)
        return grid.findGroups(linking_length, min_members)

    def groupProperties(self, catalogue: GroupCatalogue, with_potential: bool = False) -> np.ndarray:
        """fp64 properties of the groups of `catalogue` on the current bodies (GroupCatalogue.properties): mass, centre,
        bulk velocity, spin, internal kinetic energy, inertia, extent, for groups of any size.  with_potential: phi comes
        from the force method's own computePotential first, so potential is 1/2 sum m phi and phi_min_body the
        potential-minimum centre of each group in that method's model.  The bodies are not touched."""
        if not self.integrator_:
            raise ValidationException("the system is not initialised")
        d = self.d_particles_
        if catalogue.labels.numel() != d.count:
            raise ValidationException(f"the catalogue was found on {catalogue.labels.numel()} bodies, the system holds "
                                      f"{d.count}")
        phi = None
        if with_potential:
            phi = torch.empty(d.count, dtype=torch.float32, device=d.pos_x.device)
            self.force_calculator_.computePotential(d, phi)
        return catalogue.properties(d, phi, self.force_calculator_.ctx)

    # -- k nearest neighbours, local density, density centre (extension: SpatialHashGrid.neighbours) ----------------
    def localDensity(self, k: int = 6, cell=None) -> NeighbourLists:
        """The k nearest neighbours and the Casertano-Hut density of every body, for every force method, resolved by
        levels on a private grid (the force calculator's own structures are not touched): build at `cell` (default:
        neighbourCellSize), search with all outputs; while a body is unresolved -- status 1, window-limited, or status 2
        on a grid of more than 2 cells per axis -- double the cell, rebuild and refine.  A grid of at most 2 cells per
        axis resolves everything, so the loop ends by itself.  Returns a NeighbourLists (index, dist2, rho, status) with
        level [N] int32: the level that computed each body last (0 = `cell`)."""
        if not self.integrator_:
            raise ValidationException("the system is not initialised")
        d = self.d_particles_
        if cell is None:
            pos = torch.stack((d.pos_x, d.pos_y, d.pos_z))
            lo, hi = pos.min(dim=1).values.cpu().numpy(), pos.max(dim=1).values.cpu().numpy()
            cell = self.neighbourCellSize(lo, hi, d.count)
        if not (cell > 0 and _finite(cell)):
            raise ValidationException("cell must be positive and finite")
        cell = float(np.float32(cell))
        grid = self.neighbour_grid_
        if grid is None or grid.max_particles_ != d.count:
            if grid is not None:
                grid.close()
            grid = self.neighbour_grid_ = SpatialHashGrid(d.count, cell)
        grid.setCellSize(cell)
        grid.build(d)
        res = grid.neighbours(k, lists=True, density=True)
        res.level = torch.zeros(d.count, dtype=torch.int32, device=res.status.device)
        res.levels = 1
        res.cells = [cell]
        for level in range(1, 200):
            grid.ctx.synchronize()
            todo = (res.status == 1) if grid.isWholeWindow() else ((res.status == 1) | (res.status == 2))
            if not bool(todo.any()):
                break
            cell = float(np.float32(np.float32(cell) * np.float32(2)))
            grid.setCellSize(cell)
            grid.build(d)
            res.level[res.status != 0] = level
            grid.neighbours(k, lists=True, density=True, out=res)
            res.levels = level + 1
            res.cells.append(cell)
        return res

    def densityCentre(self, k: int = 6, members=None, cell=None):
        """The density centre and core radius (api.density_centre: a numpy record) of all bodies, or of the bodies
        `members`, weighted by the local density of localDensity(k, cell)."""
        res = self.localDensity(k, cell)
        return density_centre(self.force_calculator_.ctx, self.d_particles_, res.rho, members)

    # -- density-peak groups (extension: api.hop_groups) ------------------------------------------------------------
    def hopGroups(self, k: int = 16, n_hop=None, n_merge: int = 4, delta_outer=None, delta_saddle=None, delta_peak=None,
                  min_members: int = 1, cell=None) -> HopCatalogue:
        """Density-peak (HOP) groups of the bodies, for every force method: localDensity(k, cell) resolves the k nearest
        neighbours and the density of every body by doubling the cell of a private grid, then hop_groups runs on those
        lists (n_hop None: k; delta_outer None: the lower median of the densities; delta_saddle / delta_peak None: 2.5 and 3 times
        delta_outer).  Returns a HopCatalogue; its `neighbours` holds the lists and densities the groups were found
        on.  The force calculator's own structures and the bodies are not touched."""
        res = self.localDensity(k, cell)
        return _hop_on_lists(self.force_calculator_.ctx, res, n_hop, n_merge, delta_outer, delta_saddle, delta_peak,
                             min_members)

    # -- radial profiles (extension: api.groups_radial_profile) ------------------------------------------------------
    def lagrangianRadii(self, fractions=(0.1, 0.5, 0.9), k: int = 6) -> np.ndarray:
        """The radii that enclose the mass fractions `fractions` of ALL bodies as one group about densityCentre(k), for
        every force method: a float64 array, one radius per fraction."""
        centre = self.densityCentre(k)
        d = self.d_particles_
        _, shells = groups_radial_profile(self.force_calculator_.ctx, d, np.array([0, d.count], np.int32), None,
                                          np.asarray(centre["centre"], np.float64).reshape(1, 3), fractions, "mass")
        return shells["radius"][0].copy()

    def groupProfiles(self, catalogue: GroupCatalogue, cuts, mode="mass", centre: str = "com"):
        """Radial profiles of the groups of `catalogue` on the current bodies (GroupCatalogue.radialProfile) about
        centres and bulk velocities taken from groupProperties: centre "com" -- the centre of mass -- or "potential" --
        the position of phi_min_body, the potential minimum in the force method's own model.
        -> (groups, shells, properties)"""
        if centre not in ("com", "potential"):
            raise ValidationException('centre must be "com" or "potential"')
        props = self.groupProperties(catalogue, with_potential=centre == "potential")
        d = self.d_particles_
        if centre == "com":
            centres = props["com"].copy()
        else:
            body = torch.from_numpy(np.maximum(props["phi_min_body"], 0).astype(np.int64)).to(d.pos_x.device)
            centres = torch.stack((d.pos_x[body], d.pos_y[body], d.pos_z[body]), 1).to(torch.float64).cpu().numpy()
        groups, shells = catalogue.radialProfile(d, centres, cuts, mode, vels=props["vel"].copy(),
                                                 ctx=self.force_calculator_.ctx)
        return groups, shells, props
