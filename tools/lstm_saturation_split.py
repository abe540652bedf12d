#!/usr/bin/env python3
"""Where the dG error of pw_lstm_train_backward comes from at (b, N, dirs, H) = (3, 64, 1, 64), plain and with saturated gates (G x 30,
W_hh x 4: the one case of tests/test_gpu_lstm_train.py above its bound): the kernel backward fed (a) the gates the kernel forward
saved, (b) the float64 restatement's gates rounded to float32, (c) gates from torch's own float32 sigmoid / tanh; and the error of the
saved gates themselves.  Needs a GPU.

    python tools/lstm_saturation_split.py [--out profiles/lstm_train_saturated.txt]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from multiagent_rl_amd import lstm as L  # noqa: E402
from tests import lstm_ref  # noqa: E402


def err(a, ref):
    return float((a.double().cpu() - ref).abs().max())


def main():
    b, N, dirs, H = 3, 64, 1, 64
    m = lstm_ref.make_lstm(dirs, H, torch.float32, 'cuda')
    x, dY = lstm_ref.make_inputs(b, N, dirs, H, torch.float32)
    out = []
    with torch.no_grad():
        w_ih, bias, w_fw, _ = lstm_ref.projection(m)
        for gs, ws in ((1.0, 1.0), (30.0, 4.0)):
            G, W = (F.linear(x.cuda(), w_ih, bias) * gs).view(b, N, 1, 4 * H).contiguous(), (w_fw * ws).clone()
            _, sr = lstm_ref.forward(G.double().cpu(), W.double().cpu())
            dGr = lstm_ref.backward(dY.double(), sr, W.double().cpu())
            _, sk = L.launch_forward(G, W, None, True)
            _, ss = lstm_ref.forward(G, W)          # float32 with torch's own sigmoid / tanh on the GPU
            gates = lambda s: ' '.join('%.2e' % err(s[:, :, 0, q], sr[:, :, 0, q]) for q in range(5))  # noqa: E731
            out.append('G x %g, W_hh x %g: saved gates |err| i f g o c  kernel %s   torch float32 %s' % (gs, ws, gates(sk), gates(ss)))
            out.append('   dG |err|: kernel backward on kernel saved %.3e   on float64 saved rounded to float32 %.3e   on torch-float32 saved '
                       '%.3e   torch-float32 restatement end to end %.3e' % (
                           err(L.launch_backward(dY.cuda(), sk, W, None), dGr),
                           err(L.launch_backward(dY.cuda(), sr.float().cuda().contiguous(), W, None), dGr),
                           err(L.launch_backward(dY.cuda(), ss.contiguous(), W, None), dGr), err(lstm_ref.backward(dY.cuda(), ss, W), dGr)))
    text = '\n'.join(out)
    print(text)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
