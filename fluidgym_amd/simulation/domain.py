"""Batched ``Domain`` / ``Block`` / ``FixedBoundary`` facade over the HIP solver handle.

Names and call order follow the reference's PISOtorch object model so that env code reads like the
reference's (``extensions/domain_structs.h:73-802``, bindings ``extensions/PISOtorch.cpp:98-505``;
conventions in SURVEY.md Appendix B):

* faces are ``-x,+x,-y,+y,-z,+z`` = 0..2d-1, string forms accepted (``domain_structs.cpp:143-158``);
* a new block is fully periodic (``domain_structs.cpp:1161-1165``); ``CloseBoundary`` installs a
  FIXED Dirichlet boundary on the face *and* its partner (``PISOtorch.cpp:343-350``);
* every field tensor has the env batch as leading axis ``[B, C, (Z,) Y, X]`` where the reference has
  ``[1, C, ...]``; setters accept ``[1, ...]`` (broadcast over the batch) or ``[B, ...]``;
* setters copy *into* the bound device buffers, so ``UpdateDomainData()`` (which re-packs and
  re-uploads the reference's atlas, ``domain_structs.cpp:3047-3283``) is a no-op kept for
  call-compatibility.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Union

import numpy as np
import torch

from .. import _lib as L
from ..native import NativeSolver, coords_to_transforms
from . import grids

_FACE_NAMES = {"-x": 0, "+x": 1, "-y": 2, "+y": 3, "-z": 4, "+z": 5}


def face_index(face: Union[int, str]) -> int:
    if isinstance(face, str):
        return _FACE_NAMES[face]
    return int(face)


class BoundaryConditionType:
    DIRICHLET = L.FG_DIRICHLET
    NEUMANN = L.FG_NEUMANN


def _bcast_into(dst: torch.Tensor, src: torch.Tensor):
    """Copy ``src`` into ``dst`` allowing a leading batch of 1 and static ``[N, C]`` data."""
    src = src.to(device=dst.device, dtype=dst.dtype)
    if src.dim() == 2:  # static [N, C] -> broadcast over space
        src = src.reshape(src.shape[0], src.shape[1], *([1] * (dst.dim() - 2)))
    dst.copy_(src.expand_as(dst))


class FixedBoundary:
    """FIXED boundary of one face (``domain_structs.h`` FixedBoundary): Dirichlet velocity and a
    per-channel Dirichlet/Neumann passive scalar."""

    def __init__(self, block: "Block", face: int):
        self._block = block
        self.face = face
        self.passiveScalarTypes: List[int] = [BoundaryConditionType.DIRICHLET] * block.domain.n_scalars
        self._pending_velocity = None
        self._pending_scalar = None

    # tensors live in the solver once the domain is prepared
    @property
    def velocity(self) -> torch.Tensor:
        return self._block.domain.solver.bvel[self.face]

    @property
    def passiveScalar(self) -> torch.Tensor:
        return self._block.domain.solver.bscal[self.face]

    def setVelocity(self, v: torch.Tensor):
        if self._block.domain.solver is None:
            self._pending_velocity = v
        else:
            _bcast_into(self.velocity, v)

    def setPassiveScalar(self, s: torch.Tensor):
        if self._block.domain.solver is None:
            self._pending_scalar = s
        else:
            _bcast_into(self.passiveScalar, s)

    def setPassiveScalarType(self, types):
        assert self._block.domain.solver is None, "scalar boundary types are fixed at PrepareSolve()"
        self.passiveScalarTypes = [int(t) for t in types]

    # reference API parity helpers
    isVelocityStatic = False

    def makeVelocityVarying(self):  # always varying here
        return None

    def isPassiveScalarStatic(self) -> bool:
        return False

    def hasPassiveScalar(self) -> bool:
        return self._block.domain.n_scalars > 0

    def hasTransform(self) -> bool:
        return True

    def getSizes(self):
        return self._block.domain.solver.slab(self.face)

    @property
    def transform(self) -> torch.Tensor:
        """Boundary transform ``[1, slab, 2d^2+1]``; on a rectilinear grid it equals the adjacent cell
        layer's transform (``grid_gen.cu:423-452``: one-sided normal extent, tangential edge lengths)."""
        t = self._block.transform
        axis = self.face >> 1
        dim = t.dim() - 2 - axis  # spatial axis position in [1,(Z,)Y,X,T]
        idx = t.shape[dim] - 1 if (self.face & 1) else 0
        return t.narrow(dim, idx, 1)

    def GetFluxes(self) -> torch.Tensor:
        """Contravariant boundary flux ``det_b * (Minv_row_axis . u_b)`` per boundary cell ``[B, slab]``."""
        d = self._block.domain.dims
        axis = self.face >> 1
        tr = self.transform[0]
        det = tr[..., 2 * d * d]
        minv_aa = tr[..., d * d + axis * d + axis]
        return self.velocity[:, axis] * (det * minv_aa).unsqueeze(0)


class Block:
    def __init__(self, domain: "Domain", coords: torch.Tensor, name: str = "Block"):
        self.domain = domain
        self.name = name
        self.vertexCoordinates = coords
        self.edges = grids.edges_from_vertex_grid(coords)
        self.widths = [np.diff(e).astype(np.float64 if domain.dtype == torch.float64 else np.float32) for e in self.edges]
        d = domain.dims
        assert len(self.edges) == d
        self._fixed: Dict[int, FixedBoundary] = {}
        self._transform = None
        self._pending: Dict[str, torch.Tensor] = {}

    # ---- topology -------------------------------------------------------------------------
    def CloseBoundary(self, face, velocity: Optional[torch.Tensor] = None, passiveScalar: Optional[torch.Tensor] = None):
        assert self.domain.solver is None, "boundaries must be closed before PrepareSolve()"
        f = face_index(face)
        for ff in (f, f ^ 1):  # the periodic partner closes too (domain_structs.cpp:1981-2002)
            if ff not in self._fixed:
                self._fixed[ff] = FixedBoundary(self, ff)
        if velocity is not None:
            self._fixed[f].setVelocity(velocity)
        if passiveScalar is not None:
            self._fixed[f].setPassiveScalar(passiveScalar)
        return self._fixed[f]

    def getBoundary(self, face) -> FixedBoundary:
        f = face_index(face)
        if f not in self._fixed:
            raise KeyError(f"face {face} is periodic; only FIXED faces expose a boundary object")
        return self._fixed[f]

    def getFixedBoundaries(self):
        return sorted(self._fixed.items())

    def isFixed(self, face) -> bool:
        return face_index(face) in self._fixed

    # ---- fields ---------------------------------------------------------------------------
    def _field(self, name):
        return getattr(self.domain.solver, name)

    @property
    def velocity(self) -> torch.Tensor:
        return self._field("velocity")

    @property
    def pressure(self) -> torch.Tensor:
        return self._field("pressure")

    @property
    def passiveScalar(self) -> torch.Tensor:
        return self._field("scalar")

    @property
    def velocitySource(self) -> Optional[torch.Tensor]:
        return self._field("velocity_source")

    def getVelocity(self, computational: bool = False) -> torch.Tensor:
        if not computational:
            return self.velocity
        rh = self.domain.inv_widths_tensors()
        return self.velocity * rh

    def _set(self, name, t):
        if self.domain.solver is None:
            self._pending[name] = t
        else:
            _bcast_into(getattr(self.domain.solver, name), t)

    def setVelocity(self, v):
        self._set("velocity", v)

    def setPressure(self, p):
        self._set("pressure", p)

    def setPassiveScalar(self, s):
        self._set("scalar", s)

    def hasPassiveScalar(self) -> bool:
        return self.domain.n_scalars > 0

    def setVelocitySource(self, s: Optional[torch.Tensor]):
        sol = self.domain.solver
        if sol is None:
            self._pending["velocity_source"] = s
            return
        if s is None:
            sol.set_velocity_source(None)
            return
        if sol.velocity_source is None:
            sol.set_velocity_source(torch.zeros_like(sol.velocity))
        _bcast_into(sol.velocity_source, s)

    def setViscosity(self, visc: Optional[torch.Tensor]):
        """``Block.setViscosity``: a per-cell viscosity of the velocity system, ``[1 | B, 1, (Z,) Y, X]`` (the reference's layout) or
        ``[B, (Z,) Y, X]``; None returns to the domain's viscosity.  Used by the Smagorinsky hook of the TCF env
        (tcf_env.py:441-474; the kernels read it through getViscosityBlock, PISO_multiblock_cuda_kernel.cu:1816-1837)."""
        sol = self.domain.solver
        if sol is None:
            raise RuntimeError("setViscosity: PrepareSolve() first")
        if visc is None:
            sol.set_viscosity_field(None)
            return
        if getattr(sol, "viscosity_field", None) is None:
            sol.set_viscosity_field(torch.empty((sol.B,) + tuple(sol.spatial), dtype=sol.dtype, device=sol.device))
        v = visc.to(sol.device, sol.dtype)
        if v.dim() == len(sol.spatial) + 2:      # NCDHW with C = 1
            v = v[:, 0]
        sol.viscosity_field.copy_(v.expand_as(sol.viscosity_field))

    @property
    def viscosity(self) -> Optional[torch.Tensor]:
        return getattr(self.domain.solver, "viscosity_field", None)

    # ---- geometry -------------------------------------------------------------------------
    def getSizes(self):
        s = self.domain.solver
        return (s.nx, s.ny, s.nz)

    @property
    def transform(self) -> torch.Tensor:
        """``[1,(Z,)Y,X,2d^2+1]`` = M | Minv | det per cell (``domain_structs_gpu.h:160-168``), computed
        by the native ``fg_coords_to_transforms`` kernel."""
        if self._transform is None:
            dev = self.domain.device
            self._transform = coords_to_transforms(self.vertexCoordinates.to(dev, torch.float32).contiguous())
        return self._transform

    def hasTransform(self) -> bool:
        return True

    def getCellCoordinates(self) -> torch.Tensor:
        """Cell-centre coordinates ``[1, d, (Z,) Y, X]`` (mean of the cell's vertices)."""
        centers = [0.5 * (e[1:] + e[:-1]) for e in self.edges]
        d = len(centers)
        mesh = np.meshgrid(*[c for c in reversed(centers)], indexing="ij")
        c = np.stack([mesh[d - 1 - a] for a in range(d)], axis=0)[None]
        return torch.from_numpy(c).to(self.domain.device, self.domain.dtype)

    def getCellSizes(self) -> torch.Tensor:
        """Cell volumes ``[1, 1, (Z,) Y, X]`` (the determinant of the cell transform)."""
        d = self.domain.dims
        return self.transform[..., 2 * d * d].unsqueeze(1)


def per_env_values(v, batch: int, what: str):
    """``v`` as the domain keeps it: a float for one value (a number, a one-element tensor or sequence -- what it always meant), a
    float64 tensor ``[batch]`` for one value per env.  Any other length is a ``ValueError`` naming ``what``."""
    if isinstance(v, (int, float)):
        return float(v)
    t = (v.detach() if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v, dtype=np.float64))).reshape(-1).to("cpu", torch.float64)
    if t.numel() == 1:
        return float(t[0])
    if t.numel() != batch:
        raise ValueError(f"{what}: expected one value or one per env ({batch}), got {t.numel()}")
    return t.clone()


class Domain:
    """Batched stand-in for ``PISOtorch.Domain`` (one block, rectilinear grid)."""

    def __init__(self, spatialDims: int, viscosity, passiveScalarChannels: int = 0, name: str = "Domain",
                 device=None, dtype=torch.float32, batch: int = 1):
        if dtype not in (torch.float32, torch.float64):
            raise NotImplementedError("field dtype must be torch.float32 (the reference's default, fluid_env.py:146) or torch.float64")
        # torch.float64: the fields, metrics and every kernel of the step run in fp64 on the fp64 build of the library
        # (libfluidgym_hip_f64.so); the pressure CG is preconditioned by the fast-diagonalisation operator there as well (plain
        # kernels in doubles, csrc/fg_f64_fd.hip), the fp32-tuned kernel families are not part of that build
        self.dims = int(spatialDims)
        self.name = name
        self.dtype = dtype
        self.device = torch.device("cuda") if device is None else torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device() if torch.cuda.is_available() else 0)
        self.batch = int(batch)
        self.n_scalars = int(passiveScalarChannels)
        self._viscosity = per_env_values(viscosity, self.batch, "viscosity")      # float, or [B] for one value per env
        self._scalar_viscosity: Optional[list] = None
        self.blocks: List[Block] = []
        self.solver: Optional[NativeSolver] = None
        self._rh = None

    # ---- construction ---------------------------------------------------------------------
    def CreateBlock(self, vertexCoordinates: torch.Tensor, name: str = "Block") -> Block:
        if self.blocks:
            raise NotImplementedError("this class is the single-block (rectilinear) domain; connected curvilinear blocks are built "
                                      "with fluidgym_amd.simulation.multiblock.MultiBlockDomain (SURVEY 8f-3)")
        b = Block(self, vertexCoordinates, name)
        self.blocks.append(b)
        return b

    def setScalarViscosity(self, v):
        """One value per channel (``[C]``, or one element for all channels: the reference's form, read as ever), or one value per
        env and channel as an explicit 2-D ``[B, C]``."""
        tv = torch.as_tensor(v)
        if tv.dim() == 2:
            if tv.shape[1] != self.n_scalars:
                raise ValueError(f"scalar viscosity: [B, C] needs C = {self.n_scalars} channels, got {tv.shape[1]}")
            if tv.shape[0] != self.batch:
                raise ValueError(f"scalar viscosity: expected one value per env ({self.batch}), got {tv.shape[0]}")
            vals = [per_env_values(tv[:, ch], self.batch, "scalar viscosity") for ch in range(self.n_scalars)]
        else:
            flat = [float(x) for x in tv.reshape(-1)]
            vals = [flat[0] if len(flat) == 1 else flat[ch] for ch in range(self.n_scalars)]
        self._scalar_viscosity = vals
        if self.solver is not None:
            for ch in range(self.n_scalars):
                self.solver.set_scalar_viscosity(ch, vals[ch])

    @property
    def heterogeneous(self) -> bool:
        """True when the viscosity or a scalar diffusivity differs per env."""
        return isinstance(self._viscosity, torch.Tensor) or any(isinstance(k, torch.Tensor) for k in (self._scalar_viscosity or []))

    @property
    def viscosity(self) -> torch.Tensor:
        """``[1]`` (the reference's shape), or ``[B]`` when every env has its own."""
        if isinstance(self._viscosity, torch.Tensor):
            return self._viscosity.to(self.dtype)
        return torch.tensor([self._viscosity], dtype=self.dtype)

    def setViscosity(self, v):
        self._viscosity = per_env_values(v, self.batch, "viscosity")
        if self.solver is not None:
            self.solver.set_viscosity(self._viscosity)

    def PrepareSolve(self):
        """Allocate the solver workspace and bind all fields (``Domain::PrepareSolve``,
        ``domain_structs.cpp:2570-2693``)."""
        assert self.blocks, "domain has no block"
        blk = self.blocks[0]
        fixed = sorted(blk._fixed.keys())
        scalar_bc = {f: blk._fixed[f].passiveScalarTypes for f in fixed} if self.n_scalars else None
        self.solver = NativeSolver(blk.widths, self.batch, fixed_faces=fixed, n_scalars=self.n_scalars,
                                   scalar_bc=scalar_bc, device=self.device, dtype=self.dtype)
        self.solver.set_viscosity(self._viscosity)
        if self._scalar_viscosity is not None:
            for ch in range(self.n_scalars):
                self.solver.set_scalar_viscosity(ch, self._scalar_viscosity[ch])
        for name, t in blk._pending.items():
            if name == "velocity_source":
                blk.setVelocitySource(t)
            elif t is not None:
                blk._set(name, t)
        blk._pending.clear()
        for f, bnd in blk._fixed.items():
            if bnd._pending_velocity is not None:
                bnd.setVelocity(bnd._pending_velocity)
            if bnd._pending_scalar is not None and self.n_scalars:
                bnd.setPassiveScalar(bnd._pending_scalar)
            bnd._pending_velocity = bnd._pending_scalar = None
        self.solver.copy_velocity_result_from_blocks()

    def IsInitialized(self) -> bool:
        return self.solver is not None

    def UpdateDomainData(self):
        return None

    # ---- queries --------------------------------------------------------------------------
    def getBlock(self, i: int) -> Block:
        return self.blocks[i]

    def getBlocks(self):
        return list(self.blocks)

    def getNumBlocks(self) -> int:
        return len(self.blocks)

    def getSpatialDims(self) -> int:
        return self.dims

    def getDtype(self):
        return self.dtype

    def hasPassiveScalar(self) -> bool:
        return self.n_scalars > 0

    def getPassiveScalarChannels(self) -> int:
        return self.n_scalars

    def inv_widths_tensors(self) -> torch.Tensor:
        """``1/h`` per component broadcastable against ``[B, d, (Z,) Y, X]``."""
        if self._rh is None:
            blk = self.blocks[0]
            d = self.dims
            comps = []
            for a in range(d):
                shape = [1] * d
                shape[d - 1 - a] = len(blk.widths[a])
                comps.append(torch.from_numpy(1.0 / blk.widths[a]).reshape(shape).expand(*self.solver.spatial))
            self._rh = torch.stack(comps, 0).unsqueeze(0).to(self.device).contiguous()
        return self._rh

    def getMaxVelocity(self, withBounds: bool = True, computational: bool = True) -> torch.Tensor:
        """Per-env ``[B]`` (reference: scalar; ``domain_structs.cpp:1580-1611``)."""
        assert withBounds and computational, "only the variant the stepper uses is implemented natively"
        return self.solver.max_velocity()

    def GetBoundaryFluxBalance(self) -> torch.Tensor:
        return self.solver.boundary_flux_balance()

    def Clone(self, env: Optional[int] = None) -> dict:
        """State snapshot used by ``FluidEnv.get_state`` (reference: ``Domain.Clone()``); ``env``: that env alone, as a batch of one
        (an entry of a ``StateBank``)."""
        s = self.solver
        c = (lambda t: t.clone()) if env is None else (lambda t: t[int(env): int(env) + 1].clone())
        snap = {"velocity": c(s.velocity), "pressure": c(s.pressure)}
        if s.scalar is not None:
            snap["scalar"] = c(s.scalar)
        if s.velocity_source is not None:
            snap["velocity_source"] = c(s.velocity_source)
        snap["bvel"] = {f: c(t) for f, t in s.bvel.items()}
        snap["bscal"] = {f: c(t) for f, t in s.bscal.items()}
        if hasattr(s, "solver_hints"):     # which iteration the next solves run (the sweeps' back-off): part of a bit-exact replay
            snap["solver_hints"] = s.solver_hints()
        return snap

    def Restore(self, snap: dict):
        s = self.solver
        s.velocity.copy_(snap["velocity"])
        s.pressure.copy_(snap["pressure"])
        if "scalar" in snap:
            s.scalar.copy_(snap["scalar"])
        if "velocity_source" in snap and s.velocity_source is not None:
            s.velocity_source.copy_(snap["velocity_source"])
        for f, t in snap["bvel"].items():
            s.bvel[f].copy_(t)
        for f, t in snap["bscal"].items():
            s.bscal[f].copy_(t)
        if "solver_hints" in snap and hasattr(s, "solver_hints"):
            s.solver_hints(snap["solver_hints"])
        s.copy_velocity_result_from_blocks()

    def RestoreEnvs(self, bank, envs, src, flip_x=None, flip_z=None, shift_x=None, shift_z=None):
        """Restore the envs ``envs`` -- and no other -- from states of ``bank`` (a ``StateBank``): env ``envs[i]`` becomes state
        ``src[i]``, mirrored where ``flip_x[i]`` / ``flip_z[i]`` and then rolled by ``shift_x[i]`` / ``shift_z[i]`` cells
        (``torch.roll(torch.flip(t, [-1]), shift, -1)``; every argument one value or one per chosen env, None = 0).  One
        ``fg_env_restore_field`` launch per field, then ``fg_env_reset_solver_state`` for the same envs; the solver hints belong
        to the handle and stay.  Returns the selection records.  The boundary arrays of the FIXED faces get the same transform as the fields.

        A mirrored velocity component changes sign (``rbc_env_base.py:335-362``).  Pressure is transformed like a scalar: the
        reference's batch-wide randomisation (``_randomize_domain``, unchanged) leaves the pressure as it was, but here the source
        is a stored state, and a mirrored velocity next to an unmirrored pressure would be an inconsistent one.

        ``ValueError`` for what the library refuses: an index out of range, an env named twice, a shift outside ``[0, n)``, a
        mirror or roll along an axis that is not periodic (or along z in 2-D), a bank of another layout."""
        from .state_bank import build_selection

        s, blk = self.solver, self.blocks[0]
        sel = build_selection(envs, src, flip_x, flip_z, shift_x, shift_z, batch=s.B, n_states=bank.size, dims=self.dims, nx=s.nx,
                              nz=s.nz, periodic_x=not blk.isFixed(0), periodic_z=self.dims == 3 and not blk.isFixed(4))
        jobs = [(L.FG_VELOCITY, s.velocity, bank.fields["velocity"], True), (L.FG_PRESSURE, s.pressure, bank.fields["pressure"], False)]
        if s.scalar is not None and "scalar" in bank.fields:
            jobs.append((L.FG_SCALAR, s.scalar, bank.fields["scalar"], False))
        if s.velocity_source is not None and "velocity_source" in bank.fields:
            jobs.append((L.FG_VELOCITY_SOURCE, s.velocity_source, bank.fields["velocity_source"], True))
        jobs += [(L.FG_BOUND_VELOCITY + f, s.bvel[f], t, True) for f, t in bank.bvel.items()]
        jobs += [(L.FG_BOUND_SCALAR + f, s.bscal[f], t, False) for f, t in bank.bscal.items()]
        for _, dst, src_t, _ in jobs:
            if tuple(src_t.shape[1:]) != tuple(dst.shape[1:]) or src_t.dtype != dst.dtype or src_t.device != dst.device:
                raise ValueError(f"RestoreEnvs: a bank entry {tuple(src_t.shape[1:])} {src_t.dtype} on {src_t.device} does not match the "
                                 f"domain's field {tuple(dst.shape[1:])} {dst.dtype} on {dst.device}")
        for which, _, src_t, signed in jobs:
            s.env_restore_field(which, src_t, sel, signed_components=signed)
        s.env_reset_solver_state(sel)
        return sel
