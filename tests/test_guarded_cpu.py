"""The guard helper of the launch tests (tests/guarded.py) can fail: stand-in "kernels" written in torch on the CPU, one well
behaved and five sabotaged the ways a HIP kernel goes wrong at a buffer's edge.  Each sabotaged one must raise and name the buffer."""
import numpy as np
import pytest
import torch

from guarded import SENTINEL, Guard, GuardError, pointer_fields

B, H, W = 3, 4, 5


def _operands(g):
    rng = np.random.default_rng(0)
    x = g.inp('x', rng.standard_normal((B, H, W)).astype(np.float32))
    w = g.inp('w', rng.standard_normal((3, 3)).astype(np.float32))
    out = g.out('out', (B, H, W))
    return x, w, out


def _flat_with_pads(g, t):
    b = g._find(t)
    return b.alloc, b.lo, b.n


def _conv3x3(g, x, w, out, read_past_the_last_sample=False):
    """out[b] = 3x3 correlation of x[b], zero padded.  The sabotaged form stages every sample with the row that FOLLOWS it in memory
    as its bottom halo row and "masks" that row by a multiply with zero, as a kernel does that forgot the select."""
    alloc, lo, n = _flat_with_pads(g, x)
    for b in range(B):
        st = torch.zeros(H + 2, W + 2)
        st[1:H + 1, 1:W + 1] = x[b]
        if read_past_the_last_sample:
            nxt = alloc[lo + (b + 1) * H * W: lo + (b + 1) * H * W + W]          # (for b = B - 1: the first row past the tensor)
            st[H + 1, 1:W + 1] = nxt * 0.0
        acc = torch.zeros(H, W)
        for i in range(3):
            for j in range(3):
                acc += w[i, j] * st[i:i + H, j:j + W]
        out[b] = acc


def _reference(x, w):
    xp = np.pad(x.numpy(), ((0, 0), (1, 1), (1, 1)))
    return sum(w.numpy()[i, j] * xp[:, i:i + H, j:j + W] for i in range(3) for j in range(3))


def test_a_well_behaved_kernel_passes():
    g = Guard(torch, 'cpu')
    x, w, out = _operands(g)
    lab = g.inp('labels', np.array([2, 0, 1], np.int64))
    acc = g.out('acc', (4,), fill=0.0)
    raw = g.out('bytes', (7,), fill=0, dtype=torch.uint8)
    io = g.inp('state', np.ones(5, np.float32), inout=True)
    _conv3x3(g, x, w, out)
    acc += 1.0
    raw += 1
    io *= 2.0                                            # an in-out operand may change
    g.check()
    assert np.allclose(out.numpy(), _reference(x, w), atol=1e-6)
    assert lab.tolist() == [2, 0, 1]
    # payloads are aligned to 16 bytes; pads hold +inf (float inputs), 0 (integer inputs), the sentinel (outputs)
    for t, pad in ((x, float('inf')), (lab, 0), (out, SENTINEL), (raw, 0xA5)):
        alloc, lo, n = _flat_with_pads(g, t)
        assert (lo * alloc.element_size()) % 16 == 0 and lo * alloc.element_size() >= 4096
        assert bool((alloc[:lo] == pad).all()) and bool((alloc[lo + n:] == pad).all())
    # an output that feeds the next launch becomes an input: +inf pads, payload recorded
    g.freeze(out)
    alloc, lo, n = _flat_with_pads(g, out)
    assert bool(torch.isinf(alloc[:lo]).all())
    g.check()
    out[0, 0, 0] += 1.0
    with pytest.raises(GuardError, match=r'^out: input modified.*offset 0\b'):
        g.check()
    g.resnap(out)
    g.check()


def test_a_write_one_element_past_the_end_is_reported():
    g = Guard(torch, 'cpu')
    x, w, out = _operands(g)
    _conv3x3(g, x, w, out)
    alloc, lo, n = _flat_with_pads(g, out)
    alloc[lo + n] = 1.0
    with pytest.raises(GuardError, match=r'^out: written past the end.*offset %d\b' % (B * H * W)):
        g.check()


def test_a_write_one_element_before_the_start_is_reported():
    g = Guard(torch, 'cpu')
    x, w, out = _operands(g)
    _conv3x3(g, x, w, out)
    alloc, lo, n = _flat_with_pads(g, out)
    alloc[lo - 1] = 1.0
    with pytest.raises(GuardError, match=r'^out: written in front.*offset -1\b'):
        g.check()


def test_a_modified_input_is_reported():
    g = Guard(torch, 'cpu')
    x, w, out = _operands(g)
    _conv3x3(g, x, w, out)
    w[1, 2] = -w[1, 2]                                   # (a sign flip: the comparison is bit-wise)
    with pytest.raises(GuardError, match=r'^w: input modified.*offset 5\b'):
        g.check()
    g.check(payloads=False)                              # launch loops may leave the copies out; the pads are still checked
    alloc, lo, n = _flat_with_pads(g, w)
    alloc[lo + n + 3] = 0.0
    with pytest.raises(GuardError, match=r'^w: written past the end.*offset 12\b'):
        g.check(payloads=False)


def test_an_unwritten_output_element_is_reported():
    g = Guard(torch, 'cpu')
    x, w, out = _operands(g)
    _conv3x3(g, x, w, out)
    out[2, 3, 4] = float('nan')
    with pytest.raises(GuardError, match=r'^out: output not finite or left unwritten.*offset %d\b' % (B * H * W - 1)):
        g.check()


def test_a_read_past_the_last_sample_masked_by_a_multiply_is_reported():
    g = Guard(torch, 'cpu')
    x, w, out = _operands(g)
    _conv3x3(g, x, w, out, read_past_the_last_sample=True)
    assert np.allclose(out.numpy()[:B - 1], _reference(x, w)[:B - 1], atol=1e-6)       # inside the tensor the mask works
    assert not np.isfinite(out.numpy()[B - 1, H - 1]).any()                           # +inf * 0 entered the last sample's last row
    with pytest.raises(GuardError, match=r'^out: output not finite or left unwritten.*offset %d\b' % ((B - 1) * H * W + (H - 1) * W)):
        g.check()


def test_integer_and_byte_outputs_are_guarded_too():
    g = Guard(torch, 'cpu')
    idx = g.out('idx', (6,), fill=0, dtype=torch.uint8)
    alloc, lo, n = _flat_with_pads(g, idx)
    alloc[lo + n + 15] = 0
    with pytest.raises(GuardError, match=r'^idx: written past the end.*offset 21\b'):
        g.check()
    g2 = Guard(torch, 'cpu')
    ws = g2.out('workspace', (10,), fill=0.0, pad=5000)  # a workspace: pads of at least one per-sample stride
    alloc, lo, n = _flat_with_pads(g2, ws)
    assert lo >= 5000 and lo % 4 == 0
    alloc[lo + n + 4999] = 0.0
    with pytest.raises(GuardError, match=r'^workspace: written past the end.*offset 5009\b'):
        g2.check()


def test_an_output_is_due_from_the_first_launch_that_is_handed_it():
    """A test may allocate the outputs of its later launches up front: with ``touched`` (the addresses in the launch's record) an
    output's NaN fill is an error only once a launch was given the buffer -- and stays one from then on."""
    import ctypes

    class Record(ctypes.Structure):
        _fields_ = [('n', ctypes.c_int32), ('out', ctypes.c_void_p), ('aux', ctypes.c_void_p)]
    g = Guard(torch, 'cpu')
    first, second = g.out('first', (4,)), g.out('second', (4,))
    assert pointer_fields(Record(n=3, out=first.data_ptr())) == {first.data_ptr()}
    first.fill_(1.0)
    g.check(touched=pointer_fields(Record(out=first.data_ptr())))
    with pytest.raises(GuardError, match=r'^second: output not finite or left unwritten.*offset 0\b'):
        g.check(touched=pointer_fields(Record(out=first.data_ptr(), aux=second.data_ptr())))
    g.check(written=False)                               # (a pass that is not meant to fill the outputs: pads and inputs only)
    second.fill_(2.0)
    first[2] = float('nan')
    with pytest.raises(GuardError, match=r'^first: .*offset 2\b'):
        g.check(touched=set())


def test_an_infinite_output_element_and_a_pad_of_other_bits_are_reported():
    """A due output is scanned for every non-finite value, not for NaN alone; pads are compared bit for bit (-0.0 is not 0.0)."""
    g = Guard(torch, 'cpu')
    x, w, out = _operands(g)
    _conv3x3(g, x, w, out)
    out[0, 1, 0] = float('inf')
    with pytest.raises(GuardError, match=r'^out: output not finite or left unwritten.*offset %d\b' % W):
        g.check()
    g2 = Guard(torch, 'cpu')
    lab = g2.inp('labels', np.zeros(3, np.int64))
    fl = g2.out('flags', (3,), fill=0.0)
    b = g2._find(fl)
    b.padval, b.padbits = 0.0, 0
    b.alloc[:b.lo] = 0.0
    b.alloc[b.lo + b.n:] = 0.0
    g2.check()
    b.alloc[b.lo + b.n + 1] = -0.0
    with pytest.raises(GuardError, match=r'^flags: written past the end.*offset 4\b'):
        g2.check()
    assert lab.tolist() == [0, 0, 0]


def test_the_plumbing_the_launch_test_modules_share():
    import guarded
    g = guarded.begin(torch, 'cpu')
    try:
        a = guarded.dev(torch, np.arange(6, dtype=np.float32).reshape(2, 3))
        o, flat = guarded.out((2, 3)), guarded.out(5, 'scratch', fill=0.0)
        assert g._find(a).name == 'operand 0 (2, 3)' and g._find(o).name == 'output 1 (2, 3)' and tuple(flat.shape) == (5,)
        o.copy_(a)
        guarded.current.check()
        a[1, 1] = 9.0
        with pytest.raises(GuardError, match=r'^operand 0 \(2, 3\): input modified.*offset 4\b'):
            guarded.current.check()
    finally:
        guarded.end()
    z = np.array([[1 + 2j, 3 - 4j]], np.complex64)
    assert guarded.planes(z).shape == (1, 2, 2) and np.array_equal(guarded.cplx(torch.from_numpy(guarded.planes(z))), z)
    assert guarded.ptr(None) is None and guarded.ptr(a).value == a.data_ptr()
