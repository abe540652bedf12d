"""The two recurrent-weight gradients of a one-layer LSTM as include/pworld.h states them for pw_lstm_train_wgrad, in float64 and as
explicit loops over (direction, t) -- written from the header, not from the kernels and not through lstm_ref.whh_grads:

    dw_hh_fw[r][k] = sum over seq and t = 1 .. N-1 of dG[seq][t][0][r] * Y[seq][t-1][k]
    dw_hh_bw[r][k] = sum over seq and t = 0 .. N-2 of dG[seq][t][1][r] * Y[seq][t+1][H+k]

``whh_grads``: the restatement (any dtype in, float64 out).  ``launch_wgrad`` has the signature of multiagent_rl_amd.lstm.launch_wgrad,
so a CPU test can put it in that function's place; it answers in the dtype of ``dG``."""
import torch


def whh_grads(dG, Y, want_fw=True, want_bw=True):
    """dG [b,N,dirs,4H], Y [b,N,dirs*H] -> (dW_hh forward [4H,H] or None, dW_hh reverse [4H,H] or None), float64.  A step without a
    previous step in its direction is not visited at all: whatever its dG holds, NaN included, stays out."""
    b, N, dirs, H = dG.shape[0], dG.shape[1], dG.shape[2], dG.shape[3] // 4
    dG, Y = dG.detach().double().cpu(), Y.detach().double().cpu()
    out = []
    for d, want in ((0, want_fw), (1, want_bw and dirs == 2)):
        if not want:
            out.append(None)
            continue
        acc = torch.zeros(4 * H, H, dtype=torch.float64)
        for t in range(N):
            prev = t + 1 if d else t - 1
            if prev < 0 or prev >= N:
                continue
            acc += dG[:, t, d].t() @ Y[:, prev, d * H:(d + 1) * H]   # the sum over the sequences of this (direction, t)
        out.append(acc)
    return tuple(out)


def launch_wgrad(dG, Y, want_fw, want_bw):
    """Stand-in for multiagent_rl_amd.lstm.launch_wgrad (any device, any dtype)."""
    assert want_fw or want_bw
    assert not (want_bw and dG.shape[2] == 1)
    return tuple(None if g is None else g.to(device=dG.device, dtype=dG.dtype) for g in whh_grads(dG, Y, want_fw, want_bw))
