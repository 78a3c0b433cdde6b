"""Linear-operator wrappers used around the effective Hamiltonian (reference ``tenpy/linalg/sparse.py``):
``NpcLinearOperatorWrapper`` (:118), ``SumNpcLinearOperator`` (:152), ``ShiftNpcLinearOperator`` (:187),
``OrthogonalNpcLinearOperator`` (:220).  Every operation is a device call on block vectors (inner products, axpy)."""
import numpy as np

from . import _device as dev
from . import krylov_based
from . import np_conserved as npc
from .krylov_based import gram_schmidt, iadd_prefactor_other

__all__ = ['NpcLinearOperatorWrapper', 'SumNpcLinearOperator', 'ShiftNpcLinearOperator', 'OrthogonalNpcLinearOperator']


class NpcLinearOperatorWrapper:
    """Base class: everything that is not overridden is looked up on the wrapped operator."""

    def __init__(self, orig_operator):
        self.orig_operator = orig_operator

    def __getattr__(self, name):
        if name == 'orig_operator':          # (not yet set: unpickling / copy)
            raise AttributeError(name)
        return getattr(self.orig_operator, name)

    def unwrapped(self):
        op = self.orig_operator
        return op.unwrapped() if isinstance(op, NpcLinearOperatorWrapper) else op

    def matvec(self, vec):
        raise NotImplementedError("subclasses implement matvec")

    def native_input(self, theta):
        """A wrapper changes the matvec: the launch program of the wrapped operator (which ``__getattr__`` would hand out) is not the
        wrapper's.  ``None`` = the step-by-step loop, unless a subclass knows how to extend the program."""
        return None


class SumNpcLinearOperator(NpcLinearOperatorWrapper):
    """``(A + B) |vec>``."""

    def __init__(self, orig_operator, other_operator):
        super().__init__(orig_operator)
        self.other_operator = other_operator

    def matvec(self, vec):
        res = self.orig_operator.matvec(vec)
        res.iadd_prefactor_other(1., self.other_operator.matvec(vec))
        return res


class ShiftNpcLinearOperator(NpcLinearOperatorWrapper):
    """``(H + shift) |vec>``."""

    def __init__(self, orig_operator, shift):
        super().__init__(orig_operator)
        self.shift = shift

    def matvec(self, vec):
        res = self.orig_operator.matvec(vec)
        res.iadd_prefactor_other(self.shift, vec)
        return res


class OrthogonalNpcLinearOperator(NpcLinearOperatorWrapper):
    """``H -> P H P`` with ``P = 1 - sum_o |o><o|`` for the (Gram-Schmidt ortho-normalised) ``ortho_vecs``."""

    def __init__(self, orig_operator, ortho_vecs):
        super().__init__(orig_operator)
        self.ortho_vecs = gram_schmidt(list(ortho_vecs))

    def matvec(self, vec):
        vec = vec.copy(deep=True)
        for o in self.ortho_vecs:
            iadd_prefactor_other(vec, -npc.inner(o, vec, axes='range', do_conj=True), o)
        vec = self.orig_operator.matvec(vec)
        for o in self.ortho_vecs[::-1]:
            iadd_prefactor_other(vec, -npc.inner(o, vec, axes='range', do_conj=True), o)
        return vec

    def to_matrix(self):
        """``P H P`` as a matrix Array (the engines diagonalise small bonds exactly; reference :257)."""
        mat = self.orig_operator.to_matrix()
        labels = mat.get_leg_labels()
        half = len(labels) // 2
        proj = npc.eye_like(mat, 0)
        for o in self.ortho_vecs:
            o = o.combine_legs(o.get_leg_labels())
            proj = proj - npc.outer(o, o.conj())
        mat = npc.tensordot(proj, npc.tensordot(mat, proj, half), half)
        mat.iset_leg_labels(labels)
        return mat

    def adjoint(self):
        return OrthogonalNpcLinearOperator(self.orig_operator.adjoint(), self.ortho_vecs)

    def native_input(self, theta):
        """``(vector, program)`` for the native Krylov loop (``tpa_lanczos_run_ex``): the wrapped operator's launch program between two
        fused projections (op kind 4, ``tpa_project_out``) -- from the input vector into a temporary that the inner ops then read,
        and in place on the output vector: ``P H P`` as :meth:`matvec` defines it, without a host read.  ``None`` (the step-by-step
        loop; counted in ``krylov_based.stats['n_ortho_declined']`` when the ``ortho_vecs`` are the reason) if the wrapped
        operator offers no program or a sharded one, or if an ``ortho_vec`` has a block the vector's structure lacks, another
        dtype or another leg order."""
        from .. import _lib
        stats = krylov_based.stats
        if isinstance(self.orig_operator, OrthogonalNpcLinearOperator):
            return None         # (one level only: the temporary and the work area of the projections are one scratch vector each)
        make = getattr(self.orig_operator, 'native_input', None)
        got = make(theta) if make is not None else None
        if got is None:
            return None
        vec, prog = got
        ops, bufs, plans = prog[:3]
        if len(prog) > 3 or np.any(ops[:, 0] == 3) or np.any(ops[:, 0] == 4):
            return None         # collectives (sharded operators) or a program that projects already: the step-by-step route
        m = len(self.ortho_vecs)
        if m == 0:
            return got
        if m > _lib.PROJECT_MAX:
            stats['n_ortho_declined'] += 1
            return None
        n = vec._arena.numel()
        key = (vec._struct_key(), vec.dtype, tuple(vec.get_leg_labels()))
        packed = self.__dict__.get('_packed_ortho')
        if packed is None or packed[0] != key:          # once per wrapper instance and structure
            have = {tuple(r) for r in vec._qdata.tolist()}
            for o in self.ortho_vecs:
                if (o.dtype != vec.dtype or list(o.get_leg_labels()) != list(vec.get_leg_labels()) or o.rank != vec.rank
                        or any(a is not b and a != b for a, b in zip(o.legs, vec.legs))
                        or not all(tuple(r) in have for r in o._qdata.tolist())):
                    stats['n_ortho_declined'] += 1
                    return None
            basis = dev.zeros(m * n, vec.dtype)
            for j, o in enumerate(self.ortho_vecs):
                npc._scatter_blocks(o, vec, basis[j * n:(j + 1) * n])
            packed = self.__dict__['_packed_ortho'] = (key, basis)
        basis = packed[1]
        bufs = list(bufs)
        bufs += [basis, dev.scratch('ortho_in', n, vec.dtype)]
        b_slot, t_slot = len(bufs) - 2, len(bufs) - 1
        work = dev.scratch('ortho_work', 2 * m + 2 + _lib.PROJECT_WORK, np.float64).data_ptr()      # (the two projections are ordered on one stream)
        inner = np.array(ops, dtype=np.int64, copy=True)
        for col in (6, 7):
            inner[inner[:, col] == -1, col] = t_slot
        first = [4, 0, work, n, 0, m, b_slot, -1, t_slot, 0, 0, 0]
        last = [4, 0, work, n, 0, m, b_slot, -2, -2, 0, 0, 0]
        ops = np.concatenate([np.array([first], dtype=np.int64), inner, np.array([last], dtype=np.int64)])
        stats['n_native_ortho'] += 1
        return vec, (ops, bufs, plans)
