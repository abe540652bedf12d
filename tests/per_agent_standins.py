"""Test infrastructure (never imported by the product): the per-agent form of tests/dist_standins.py -- torch restatements of the
``pw_replay_add_*wire_agents`` launches, so that ``FullTransitionGather(per_agent=True)`` can run with the gloo backend on CPU tensors
(tests/test_per_agent_wire_gloo.py).  The GPU parity of the real launches is in tests/test_gpu_per_agent_wire.py."""
import torch

from tests.dist_standins import STANDINS, CpuFullGather, HostRing, HostStateRing


def agents_transitions_reference(g, block):
    """``pw_replay_add_*wire_agents``: the block's T*B transitions exactly as the plain entry point writes them, with ``rew`` [T*B, N] read
    from the trailer plane behind the block (NOT from its rew_shared plane) and ``done`` [T*B, N] = 0."""
    tr = STANDINS[g.format.Struct.__name__][1](g, block)
    T, B, N = g.T, g.B, g.N
    trailer = block[g.lay.total_bytes:g.lay.total_bytes + 4 * T * B * N].view(torch.float32)
    tr['rew'] = trailer.reshape(T * B, N).clone()
    tr['done'] = torch.zeros(T * B, N)
    return tr


class CpuPerAgentGather(CpuFullGather):
    """``FullTransitionGather(per_agent=True)`` with torch stand-ins for its launches; the ring is a host ring marked per-agent."""

    def _make_memory(self):
        m = HostStateRing(self.scenario, self.A) if self.ring_kind == 'state' else HostRing()
        m.per_agent = True
        return m

    def _ingest(self, block):
        assert self.per_agent and block.numel() == self.block_bytes > self.lay.total_bytes
        tr = agents_transitions_reference(self, block)
        if isinstance(self.memory, HostStateRing):
            self.memory.append(tr)
        else:
            self.memory.transitions.append(tr)
