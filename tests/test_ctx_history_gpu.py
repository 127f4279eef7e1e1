"""Every call after every other on one context (tests/ctx_history.py, part 2).

The session-wide Engine of tests/conftest.py makes every other GPU test run on whatever its predecessors left in the context; here the
history is the test's own.  The catalogue holds N = 52 nodes (operation, grid side), each with deterministic inputs and an expectation
computed on the CPU by the reference its feature's own test uses.  One Eulerian circuit of the complete digraph on the nodes, self-loops
included, orders N^2 = 2704 calls so that EVERY ordered pair (previous call, this call) occurs exactly once: grow, shrink and repeat of every
operation after every operation -- pairs, not longer histories (those occur only as the circuit happens to contain them).  The circuit is
cut into chunks; each runs on a fresh context and begins with the node the chunk before ended with.

Every output is compared ON THE DEVICE, bit for bit (integer views), with the uploaded expectation -- 16 elements of pattern behind every
output included -- and one word per (call, output) goes into a tensor that is read back once per chunk; counts that come back on the host
are compared as they come.  Two traversals: "sync" waits after every call (every lazily copied count has landed before the next call),
"prof" never waits and brackets every kernel with events (counts land late or never; the ProfScope paths run).  A failure names the pair
`previous node -> node`, the output and the first differing index."""
import os
import sys

import numpy as np
import pytest
import torch

from cuda_mesh_voxelization_amd import capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ctx_history as H  # noqa: E402

pytestmark = pytest.mark.gpu

PATTERN = 0x5A5A5A5A
EQUAL = (1 << 62)
WALK = H.euler_circuit(len(H.CATALOGUE))
CHUNKS = H.chunks(WALK)
MAX_OUTPUTS = 3


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"
    return torch.device("cuda", 0)


def _bits(a):
    a = np.array(a, copy=True).reshape(-1)                               # (a copy: the cached arrays are read-only)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


@pytest.fixture(scope="module")
def world(dev):
    """Per node: the uploaded inputs, the expectations (padded with the pattern) and the output buffers.  Computed and uploaded once."""
    w = []
    for node in H.CATALOGUE:
        dev_exp, host_exp = node.expected()
        assert len(dev_exp) <= MAX_OUTPUTS
        I = {k: torch.from_numpy(_bits(v).reshape(np.asarray(v).shape)).to(dev) for k, v in node.inputs().items()}
        E, Out = {}, {}
        for k, v in dev_exp.items():
            b = _bits(v)
            pad = np.full(H.SLACK * 4 // b.dtype.itemsize, PATTERN if b.dtype == np.int32 else (PATTERN << 32) | PATTERN, b.dtype)
            E[k] = torch.from_numpy(np.concatenate([b, pad])).to(dev)
            Out[k] = torch.empty_like(E[k])
        w.append((node, I, E, Out, host_exp))
    return w


@pytest.mark.parametrize("chunk", range(len(CHUNKS)), ids=lambda i: "chunk%d" % i)
@pytest.mark.parametrize("mode", ["sync", "prof"])
def test_every_call_after_every_other(dev, world, mode, chunk):
    walk = CHUNKS[chunk]
    results = torch.full((len(walk), MAX_OUTPUTS), EQUAL, dtype=torch.int64, device=dev)
    ramps = {}
    failures = []
    ctx = capi.Context(0)
    try:
        ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream, external=True)
        if mode == "prof":
            ctx.prof_select(None)
            ctx.prof_enable(True)
        prev = "(fresh context)"
        for c, idx in enumerate(walk):
            node, I, E, Out, host_exp = world[idx]
            for t in Out.values():
                t.view(torch.int32).fill_(PATTERN)
            try:
                host = node.run(ctx, I, Out)
            except capi.VPError as e:
                if e.code < 10000:
                    raise                                                # a HIP error: nothing more is started on the device
                failures.append("%s -> %s: %s" % (prev, node.name, e))
                host = None
            if host is not None and host != host_exp:
                failures.append("%s -> %s: host values %s, expected %s" % (prev, node.name, host, host_exp))
            for j, k in enumerate(E):
                neq = Out[k] != E[k]
                m = neq.numel()
                if m not in ramps:
                    ramps[m] = torch.arange(m, dtype=torch.int64, device=dev)
                results[c, j] = torch.where(neq, ramps[m], EQUAL).min()
            if mode == "sync":
                ctx.sync()
            prev = node.name
        if mode == "prof":
            ctx.prof_enable(False)
            assert ctx.prof(), "no kernel was timed"
        ctx.sync()
        got = results.cpu().numpy()                                     # the one read-back of the chunk
    finally:
        ctx.close()
    for c, j in zip(*np.nonzero(got != EQUAL)):
        node = world[walk[c]][0]
        prev = world[walk[c - 1]][0].name if c else "(fresh context)"
        failures.append("%s -> %s: output %s differs first at index %d" % (prev, node.name, list(world[walk[c]][2])[j], got[c, j]))
    assert not failures, "%d of %d calls wrong (%s): %s" % (len(failures), len(walk), mode, "; ".join(failures[:20]))
