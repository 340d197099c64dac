"""The float64 reference the GPU sequence tests compare against (`oracle/blvm_oracle.py::lstm_sequence_ref`, the contract of
`blvm_lstm_seq_fwd` in include/blvm_hip.h) is itself pinned here, without a GPU:
  * against `nn.LSTM` on `pack_padded_sequence(enforce_sorted=False)` with a non-zero initial state, where packing can express the
    lengths (unsorted, >= 1): outputs, final states and every gradient to 1e-12 absolute (the two agree to a few 1e-15);
  * on what packing cannot express — a row of length 0 — by the properties the contract states, exactly;
  * `lens=None` is the same as every row at full length."""
import torch

import blvm_oracle as O

T_, B, I, H = 7, 21, 16, 48
ATOL = 1e-12


def _case(seed=11):
    g = torch.Generator().manual_seed(seed)
    lstm = torch.nn.LSTM(I, H).double()
    with torch.no_grad():
        for p in lstm.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.3)
    x = torch.randn(T_, B, I, generator=g, dtype=torch.float64)
    h0 = torch.randn(B, H, generator=g, dtype=torch.float64) * 0.5
    c0 = torch.randn(B, H, generator=g, dtype=torch.float64) * 0.5
    w = torch.randn(T_, B, H, generator=g, dtype=torch.float64)
    return lstm, x, h0, c0, w


def _params(lstm):
    return lstm.weight_ih_l0, lstm.weight_hh_l0, lstm.bias_ih_l0, lstm.bias_hh_l0


def _run_ref(lstm, x, h0, c0, lens, w):
    """-> (out, h_n, c_n), [d_x, d_h0, d_c0, dWih, dWhh, dbih, dbhh] of loss = (out * w).sum() through the reference loop."""
    leaves = [t.clone().requires_grad_(True) for t in (x, h0, c0)] + [p.detach().clone().requires_grad_(True) for p in _params(lstm)]
    out, hn, cn = O.lstm_sequence_ref(leaves[0], leaves[1], leaves[2], lens, *leaves[3:])
    (out * w).sum().backward()
    return (out.detach(), hn.detach(), cn.detach()), [t.grad for t in leaves]


def test_reference_loop_equals_packed_nn_lstm_with_initial_state():
    lstm, x, h0, c0, w = _case()
    lens = torch.tensor([(5 * k + 3) % T_ + 1 for k in range(B)])  # unsorted, 1 .. T
    assert lens.min() == 1 and lens.max() == T_ and not bool((lens[:-1] >= lens[1:]).all())
    (out, hn, cn), grads = _run_ref(lstm, x, h0, c0, lens, w)

    xr, h0r, c0r = (t.clone().requires_grad_(True) for t in (x, h0, c0))
    ps = torch.nn.utils.rnn.pack_padded_sequence(xr, lens, enforce_sorted=False)
    po, (phn, pcn) = lstm(ps, (h0r.unsqueeze(0), c0r.unsqueeze(0)))
    pout, _ = torch.nn.utils.rnn.pad_packed_sequence(po, total_length=T_)
    (pout * w).sum().backward()
    want = [xr.grad, h0r.grad, c0r.grad] + [p.grad for p in _params(lstm)]

    for name, a, b in (("out", out, pout), ("h_n", hn, phn[0]), ("c_n", cn, pcn[0])):
        assert float((a - b.detach()).abs().max()) < ATOL, name
    for name, a, b in zip(("d_x", "d_h0", "d_c0", "dWih", "dWhh", "dbih", "dbhh"), grads, want):
        assert float((a - b).abs().max()) < ATOL, name
    for b in range(B):  # zero past each row's length, exactly
        assert bool((out[int(lens[b]):, b] == 0).all()), b


def test_reference_loop_length_zero_row_is_untouched_exactly():
    lstm, x, h0, c0, w = _case(seed=12)
    lens = torch.tensor([(5 * k + 3) % T_ + 1 for k in range(B)])
    dead = (4, 17)
    for b in dead:
        lens[b] = 0
    (out, hn, cn), (d_x, d_h0, d_c0, *_) = _run_ref(lstm, x, h0, c0, lens, w)
    for b in dead:
        assert bool((out[:, b] == 0).all())
        assert torch.equal(hn[b].view(torch.int64), h0[b].view(torch.int64))  # bit for bit
        assert torch.equal(cn[b].view(torch.int64), c0[b].view(torch.int64))
        assert bool((d_x[:, b] == 0).all()) and bool((d_h0[b] == 0).all()) and bool((d_c0[b] == 0).all())
    live = [b for b in range(B) if b not in dead]
    assert bool((d_h0[live].abs().amax(1) > 0).all()) and bool((d_c0[live].abs().amax(1) > 0).all())


def test_reference_loop_without_lengths_or_state():
    lstm, x, h0, c0, w = _case(seed=13)
    full = torch.full((B,), T_)
    with torch.no_grad():
        a = O.lstm_sequence_ref(x, h0, c0, None, *_params(lstm))
        b = O.lstm_sequence_ref(x, h0, c0, full, *_params(lstm))
        z = O.lstm_sequence_ref(x, None, None, None, *_params(lstm))
        zz = O.lstm_sequence_ref(x, torch.zeros_like(h0), torch.zeros_like(c0), full, *_params(lstm))
        ref, (rh, rc) = lstm(x, (h0.unsqueeze(0), c0.unsqueeze(0)))
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    for u, v in zip(z, zz):
        assert torch.equal(u, v)
    assert float((a[0] - ref).abs().max()) < ATOL and float((a[1] - rh[0]).abs().max()) < ATOL and float((a[2] - rc[0]).abs().max()) < ATOL
