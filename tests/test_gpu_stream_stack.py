"""GPU test of the one streaming stack (stream_stack.StreamStack): a clip cut into chunks and carried through ALL groups of
the plan by ``launch_groups`` and the classifier's roll launch leaves, in the stored z and in ``top``, the bits of the
whole-clip group kernel run once per group of the same plan -- test_gpu_recognizer's test_z_stream_form_keeps_the_bits carried
from one group to the stack -- at the clock and, on the same inputs, in the slot form on a table [t, t + n] per slot."""
import numpy as np
import pytest
import torch

from oracle import wavenet_np as O
from tests._pkg import sub
from tests.test_gpu_kernels import DEV, dev

pytestmark = pytest.mark.gpu

DIL = [1, 2, 4, 8, 16, 32, 64]
B, CHUNKS, MAX_CHUNK, S = 2, (40, 160, 1, 40), 160, 128


def _bits(t):
    return t.contiguous().view(torch.uint8)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("R", [32, 64])
def test_stack_stream_keeps_the_bits_of_the_whole_clip(R, dt):
    R_, K, L_, SK = sub("recognizer"), sub("kernels"), sub("_lib"), sub("stream_stack")
    L, T = len(DIL), sum(CHUNKS)
    w = R_.ClassifierWeights(DIL, R, S, 12, 2, dt)
    w.load_oracle_params(O.init_stack_params(3, DIL, 2, R, S, 12, bias_scale=0.1))
    x0 = torch.tensor(np.random.default_rng(R).normal(0, 0.5, size=(B, T, R)), dtype=dt, device=DEV)
    clock_sk, slots_sk = (SK.StreamStack(w, B, MAX_CHUNK, store_z=True) for _ in range(2))
    groups, hist, G = clock_sk.groups, clock_sk.hist, len(clock_sk.groups)
    assert G >= 2 and slots_sk.groups == groups
    # the whole clip, once per group of the same plan: a group's output is the next group's input
    x_whole = torch.zeros((L, B, T, R), dtype=dt, device=DEV)
    z_whole = torch.zeros((L, B, T, R), dtype=dt, device=DEV)
    x_in = x0
    for l0, l1 in groups:
        K.residual_group_fwd(x_in, x_whole[l0:l1], z_whole[l0:l1], [w.wptr(o) for o in w.o_conv[l0:l1]],
                             [w.wptr(o) for o in w.o_res[l0:l1]], [w.view("BF")[l] for l in range(l0, l1)],
                             [w.view("BR")[l] for l in range(l0, l1)], DIL[l0:l1])
        x_in = x_whole[l1 - 1]
    torch.cuda.synchronize()
    clock = torch.zeros(1, dtype=torch.int64, device=DEV)
    table = torch.zeros((B, 2), dtype=torch.int64, device=DEV)
    xbuf, carry = torch.zeros((B, MAX_CHUNK), device=DEV), torch.zeros(B, device=DEV)      # the roll's audio: not looked at
    tail = (MAX_CHUNK, R, K.abi_dtype(dt), K._stream())
    t = 0
    for n in CHUNKS:
        table.copy_(torch.tensor([[t, t + n]] * B, dtype=torch.int64))
        for sk in (clock_sk, slots_sk):
            sk.bufs[0][:, hist[0]:hist[0] + n] = x0[:, t:t + n]
            sk.zs.fill_(float("nan")); sk.top.fill_(float("nan"))
        clock_sk.launch_groups(B, n, clock.data_ptr())
        L_.call("srwn_recog_roll", clock_sk.roll.data_ptr(), G, xbuf.data_ptr(), MAX_CHUNK, carry.data_ptr(), clock.data_ptr(),
                B, n, *tail)
        slots_sk.launch_groups(B, n, table.data_ptr(), slots=True)
        L_.call("srwn_recog_roll_slots", slots_sk.roll.data_ptr(), G, table.data_ptr(), B, n, *tail)
        torch.cuda.synchronize()
        assert int(clock) == t + n
        for what, sk in (("clock", clock_sk), ("slots", slots_sk)):
            assert torch.equal(_bits(sk.zs[:, :B, :n]), _bits(z_whole[:, :, t:t + n])), (what, t, n)
            assert torch.equal(_bits(sk.top[:B, :n]), _bits(x_whole[L - 1][:, t:t + n])), (what, t, n)
            assert torch.isnan(sk.zs[:, :, n:].float()).all() and torch.isnan(sk.top[:, n:].float()).all()      # nothing behind
        t += n
