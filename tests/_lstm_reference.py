"""The float64 recurrences the LSTM kernels (csrc/lstm.hip) are tested against, on the CPU: the forward of torch.nn.LSTM
(model.py:91-110) layer by layer, and the backward of one layer from the saved gate activations and cell states.  Shared by
tests/test_gpu_demucs.py, tests/test_gpu_demucs_train.py and tests/test_gpu_lstm.py."""
import torch


def lstm_layer_forward(xp, whh):
    """One layer from its input projections xp (B, Tn, 4H) = x W_ih^T + b and W_hh (4H, H), zero initial state
    -> (h (B, Tn, H), c (B, Tn, H), gate activations [sig i | sig f | tanh g | sig o] (B, Tn, 4H)), float64."""
    B, Tn, H4 = xp.shape
    H = H4 // 4
    W = whh.double().t()
    h = torch.zeros(B, H, dtype=torch.float64)
    c = torch.zeros(B, H, dtype=torch.float64)
    hs, cs, gs = [], [], []
    for t in range(Tn):
        g = xp[:, t].double() + h @ W
        i, f, gg, o = g.split(H, dim=1)
        i, f, gg, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(gg), torch.sigmoid(o)
        c = f * c + i * gg
        h = o * torch.tanh(c)
        hs.append(h)
        cs.append(c)
        gs.append(torch.cat([i, f, gg, o], dim=1))
    return torch.stack(hs, dim=1), torch.stack(cs, dim=1), torch.stack(gs, dim=1)


def lstm_reference(x, skip, wih, bias, whh):
    """torch.nn.LSTM's recurrence (model.py:91-110) in float64 on the CPU: two layers, then + skip."""
    inp = x.double()
    for k in range(2):
        inp = lstm_layer_forward(inp @ wih[k].double().t() + bias[k].double(), whh[k])[0]
    return inp + skip.double()


def lstm_layer_backward(gates, cseq, dhout, whh):
    """The backward recurrence of one layer in float64: gates (B, Tn, 4H) = the saved activations [sig i | sig f | tanh g | sig o],
    cseq / dhout (B, Tn, H), W_hh (4H, H) -> (gradients of the gate pre-activations (B, Tn, 4H), dc after step 0 (B, H))."""
    B, Tn, H = cseq.shape
    W = whh.double()
    dgn = torch.zeros(B, 4 * H, dtype=torch.float64)
    dc = torch.zeros(B, H, dtype=torch.float64)
    want = torch.zeros(B, Tn, 4 * H, dtype=torch.float64)
    for t in range(Tn - 1, -1, -1):
        vi, vf, vg, vo = [x.double() for x in gates[:, t].split(H, dim=1)]
        ct = cseq[:, t].double()
        cp = cseq[:, t - 1].double() if t else torch.zeros_like(ct)
        dh = dhout[:, t].double() + dgn @ W
        tc = torch.tanh(ct)
        dO = dh * tc * vo * (1 - vo)
        dcv = dc + dh * vo * (1 - tc * tc)
        di = dcv * vg * vi * (1 - vi)
        df = dcv * cp * vf * (1 - vf)
        dg = dcv * vi * (1 - vg * vg)
        dc = dcv * vf
        dgn = torch.cat([di, df, dg, dO], dim=1)
        want[:, t] = dgn
    return want, dc
