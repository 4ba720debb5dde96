"""NumPy oracles of the No-U-Turn draw (hamiltonian_monte_carlo/nuts.py) on an
identity mass matrix, in two forms:

  * `Tree`: a recursive restatement of _TrajectoryTree -- a half-tree of height
    h is a half-tree of height h - 1 that, unless it terminated, absorbs a
    second one grown from its far end;
  * `unrolled_half_tree`: the schedule the device runs (csrc/cox.hip): the
    steps t = 1 .. 2^h in a row; after step t a singleton, then, while
    2^(l+1) divides t, the pending tree of height l absorbs the tree of
    height l just completed; a tree lives in the buffer of its first leaf;
    a terminated tree folds its flags and min / max Hamiltonian into the
    pending trees on its left and the remaining steps are not taken.

Both draw the merges' uniforms from `uniform()`, a callable, so a test can
feed one sequence to both and count what was consumed.  `generate_next_state`
is NoUTurnSampler.generate_next_state on the global NumPy stream."""
import math

import numpy as np


def leapfrog(f, dt, q, p, grad):
    """dynamics.py velocity_verlet, identity mass."""
    p = p + 0.5 * dt * grad
    q = q + dt * p
    logp, grad = f(q)
    if math.isfinite(logp):
        p = p + 0.5 * dt * grad
    return q, p, logp, grad


def hamiltonian(logp, p):
    return -logp + 0.5 * np.dot(p, p)


class Shared:
    """What every tree of one draw shares."""

    def __init__(self, f, dt, init_joint, threshold, tol, uniform):
        self.f, self.dt = f, dt
        self.init_joint, self.threshold, self.tol = init_joint, threshold, tol
        self.uniform = uniform
        self.n_step = 0
        self.n_uniform = 0

    def draw(self):
        self.n_uniform += 1
        return self.uniform()


class Tree:
    def __init__(self, sh, q, p, logp, grad, joint):
        self.sh = sh
        self.front = self.rear = (q, p, grad)
        self.sample = (q, logp, grad)
        self.u_turn = False
        self.hmin = self.hmax = -joint
        self.n_acc = int(joint > sh.threshold)
        self.height = 0
        self.err = abs(sh.init_joint - joint)
        self.acc = min(1, math.exp(joint - sh.init_joint))

    @property
    def unstable(self):
        return (self.hmax - self.hmin) > self.sh.tol

    @property
    def terminated(self):
        return self.u_turn or self.unstable

    def end(self, d):
        return self.front if d > 0 else self.rear

    def singleton(self, q, p, grad, d):
        sh = self.sh
        q, p, logp, grad = leapfrog(sh.f, d * sh.dt, q, p, grad)
        sh.n_step += 1
        joint = -math.inf if math.isinf(logp) else -hamiltonian(logp, p)
        return Tree(sh, q, p, logp, grad, joint)

    def build(self, q, p, grad, height, d):
        if height == 0:
            return self.singleton(q, p, grad, d)
        sub = self.build(q, p, grad, height - 1, d)
        if not sub.terminated:
            sub.merge(sub.build(*sub.end(d), height - 1, d), d, 'uniform')
        return sub

    def double(self, height, d):
        return self.merge(self.build(*self.end(d), height, d), d, 'swap')

    def merge(self, nxt, d, method):
        self.u_turn = self.u_turn or nxt.u_turn
        self.hmin = min(self.hmin, nxt.hmin)
        self.hmax = max(self.hmax, nxt.hmax)
        rejected = nxt.terminated
        if not rejected:
            if method == 'uniform':
                w = nxt.n_acc / max(1, self.n_acc + nxt.n_acc)
            else:
                w = nxt.n_acc / self.n_acc
            if self.sh.draw() < w:
                self.sample = nxt.sample
            self.n_acc += nxt.n_acc
            if d > 0:
                self.front = nxt.front
            else:
                self.rear = nxt.rear
            dq = self.front[0] - self.rear[0]
            self.u_turn = self.u_turn or bool(
                np.dot(dq, self.front[1]) < 0 or np.dot(dq, self.rear[1]) < 0)
            n, m = 2 ** self.height, 2 ** nxt.height
            w = n / (n + m)
            self.err = w * self.err + (1 - w) * nxt.err
            self.acc = w * self.acc + (1 - w) * nxt.acc
            self.height += 1
        return rejected


def tree_scalars(t):
    return dict(u_turn=bool(t.u_turn), hmin=t.hmin, hmax=t.hmax,
                n_acc=t.n_acc, height=t.height, err=t.err, acc=t.acc,
                sample_logp=t.sample[1])


def buffer_of(i, h):
    """The buffer of the tree whose first leaf has the 0-based index i."""
    return h if i == 0 else (i & -i).bit_length() - 1


class _Slot:
    """A tree as the device keeps it: scalars, the near end, the sample."""


def unrolled_half_tree(sh, q, p, grad, h, d):
    """The device's schedule for one half-tree.  Returns (tree scalars as
    `tree_scalars`, sample (q, logp, grad), far end (q, p, grad), stopped)."""
    slots = {}
    stop = False

    def flags(t, a):
        t.u_turn = t.u_turn or a.u_turn
        t.hmin = min(t.hmin, a.hmin)
        t.hmax = max(t.hmax, a.hmax)

    def terminated(t):
        return t.u_turn or (t.hmax - t.hmin) > sh.tol

    for t in range(1, 2 ** h + 1):
        q, p, logp, grad = leapfrog(sh.f, d * sh.dt, q, p, grad)
        sh.n_step += 1
        joint = -math.inf if math.isinf(logp) else -hamiltonian(logp, p)
        leaf = _Slot()
        leaf.u_turn, leaf.hmin, leaf.hmax = False, -joint, -joint
        leaf.n_acc, leaf.height = int(joint > sh.threshold), 0
        leaf.err = abs(sh.init_joint - joint)
        leaf.acc = min(1, math.exp(joint - sh.init_joint))
        leaf.near = (q, p)
        leaf.sample = (q, logp, grad)
        if t & 1:
            slots[buffer_of(t - 1, h)] = leaf
            continue
        done = leaf                    # the tree just completed, height l
        lev = 0
        while lev < h and t % (2 << lev) == 0:
            first = t - (2 << lev)
            pend = slots[buffer_of(first, h)]
            assert pend.height == done.height == lev
            assert lev == 0 or done is slots[lev]
            flags(pend, done)
            if sh.draw() < done.n_acc / max(1, pend.n_acc + done.n_acc):
                pend.sample = done.sample
            pend.n_acc += done.n_acc
            (qf, pf), (qr, pr) = ((q, p), pend.near) if d > 0 \
                else (pend.near, (q, p))
            dq = qf - qr
            if np.dot(dq, pf) < 0 or np.dot(dq, pr) < 0:
                pend.u_turn = True
            n, m = 2 ** pend.height, 2 ** done.height
            w = n / (n + m)
            pend.err = w * pend.err + (1 - w) * done.err
            pend.acc = w * pend.acc + (1 - w) * done.acc
            pend.height += 1
            if terminated(pend):
                cur, i = pend, first
                while i > 0:
                    i -= i & -i
                    left = slots[buffer_of(i, h)]
                    flags(left, cur)
                    cur = left
                stop = True
                break
            done = pend
            lev += 1
        if stop:
            break
    res = slots[h]
    return tree_scalars(res), res.sample, (q, p, grad), stop


def generate_next_state(f, dt, q, logp, grad, p=None, max_height=10,
                        tol=100., uniform=None):
    """NoUTurnSampler.generate_next_state (nuts.py:108-151) on the global
    NumPy stream.  Returns (q, info); info['uniforms'] lists the uniforms the
    merges consumed and info['doublings'] the per-doubling records."""
    if p is None:
        p = np.random.randn(len(q))
    joint = -hamiltonian(logp, p)
    threshold = joint - np.random.exponential()
    directions = 2 * (np.random.rand(max_height) < 0.5) - 1
    used = []

    def draw():
        used.append(np.random.uniform() if uniform is None else uniform())
        return used[-1]
    sh = Shared(f, dt, joint, threshold, tol, draw)
    tree = Tree(sh, q, p, logp, grad, joint)
    height, doublings = 0, []
    while True:
        before = (sh.n_step, sh.n_uniform)
        rejected = tree.double(height, directions[height])
        doublings.append(dict(rejected=rejected,
                              n_steps=sh.n_step - before[0],
                              n_uniform=sh.n_uniform - before[1],
                              **tree_scalars(tree)))
        height += 1
        if tree.u_turn or tree.unstable or height >= max_height:
            break
    q, logp, grad = tree.sample
    info = dict(logp=logp, grad=grad, ave_accept_prob=tree.acc,
                ave_hamiltonian_error=tree.err, n_grad_evals=sh.n_step,
                tree_height=height, u_turn_detected=bool(tree.u_turn),
                instability_detected=bool(tree.unstable),
                last_doubling_rejected=bool(rejected),
                directions=directions, uniforms=np.array(used),
                n_uniform=len(used), doublings=doublings, momentum=p)
    return q, info
