"""What ``sbc_ldamp_create``, ``sbc_wgan_create`` and ``sbc_score_create`` refuse before they touch a device: every case returns
``SBC_ERR_INVALID`` and leaves a message that starts with the function's name and quotes the facts (tensor name, element counts).
No GPU needed: none of these paths reaches a HIP call."""
import ctypes as C

import numpy as np
import pytest

from score_based_channels_amd import _lib, ldamp, wgan

SBC_ERR_INVALID = -1
LDAMP_FIRST = 'update_nets.0.unet.down_sample_layers.0.layers.0.weight'


def _refuses(call, function, *facts):
    """``call(refs..., byref(handle))`` must return SBC_ERR_INVALID without a handle; the error names ``function`` and every fact."""
    h = C.c_void_p()
    rc = call(C.byref(h))
    msg = _lib.lib().sbc_last_error().decode()
    assert rc == SBC_ERR_INVALID, (rc, msg)
    assert h.value is None
    assert msg.startswith(function + ':'), msg
    for fact in facts:
        assert str(fact) in msg, (fact, msg)
    return msg


def _ldamp(sd, names=None, n_nets=1, n_tensors=None, edit=None):
    refs, keep = _lib.tensor_refs(sd, list(sd) if names is None else names)
    if edit:
        edit(refs)
    n = len(refs) if n_tensors is None else n_tensors
    return lambda out: _lib.lib().sbc_ldamp_create(refs, n, n_nets, out), keep


def _wgan(sd, names=None, n_tensors=None, edit=None):
    refs, keep = _lib.tensor_refs(sd, list(sd) if names is None else names)
    if edit:
        edit(refs)
    n = len(refs) if n_tensors is None else n_tensors
    return lambda out: _lib.lib().sbc_wgan_create(refs, n, out), keep


def _score(sd, conv_mode=3, flags=0x3f, edit=None):
    refs, keep = _lib.tensor_refs(sd, [k for k in sd if k != 'sigmas'])
    if edit:
        edit(refs)
    sig = np.ascontiguousarray(sd['sigmas'], np.float32)
    desc = _lib.sbc_score_desc(ngf=32, channels=2, nt=64, nr=16, batch=1, conv_mode=conv_mode, sigmas=sig.ctypes.data,
                               num_classes=sig.size, flags=flags)
    return lambda out: _lib.lib().sbc_score_create(C.byref(desc), refs, len(refs), out), (keep, sig, desc)


def _no_name(refs):
    refs[1].name = None


def _no_data(refs):
    refs[1].data = None


@pytest.fixture(scope='module')
def ldamp_sd():
    return ldamp.seeded_state_dict(1, 1)


@pytest.fixture(scope='module')
def wgan_sd():
    return {k: v for k, v in wgan.seeded_state_dict(1, 1).items() if not k.endswith('num_batches_tracked')}


def test_ldamp_create_refuses_a_wrong_tensor_count():
    call, keep = _ldamp({'x': np.zeros(4)})
    _refuses(call, 'sbc_ldamp_create', '1 nets have 19 tensors (got 1)')


def test_ldamp_create_refuses_a_renamed_tensor(ldamp_sd):
    sd = dict(ldamp_sd)
    sd['bogus'] = sd.pop(LDAMP_FIRST)
    call, keep = _ldamp(sd)
    _refuses(call, 'sbc_ldamp_create', LDAMP_FIRST)


def test_ldamp_create_refuses_one_element_too_many(ldamp_sd):
    assert ldamp_sd[LDAMP_FIRST].size == 288
    call, keep = _ldamp(dict(ldamp_sd, **{LDAMP_FIRST: np.zeros(289)}))
    _refuses(call, 'sbc_ldamp_create', LDAMP_FIRST, '289', '288')


def test_ldamp_create_refuses_a_name_given_twice(ldamp_sd):
    names = list(ldamp_sd)
    call, keep = _ldamp(ldamp_sd, [names[0]] + names[:1] + names[2:])
    _refuses(call, 'sbc_ldamp_create', names[0], 'twice')


def test_wgan_create_refuses_a_short_dense_bias(wgan_sd):
    call, keep = _wgan(dict(wgan_sd, **{'dense.dense_input.bias': np.zeros(3)}))
    _refuses(call, 'sbc_wgan_create', 'dense.dense_input.bias', '3', '8192')


def test_wgan_create_refuses_a_name_given_twice(wgan_sd):
    names = list(wgan_sd)
    assert names[0] == 'dense.dense_input.weight'
    call, keep = _wgan(wgan_sd, [names[0]] + names[:1] + names[2:])
    _refuses(call, 'sbc_wgan_create', 'dense.dense_input.weight', 'twice')


def test_wgan_create_refuses_one_tensor_short(wgan_sd):
    assert len(wgan_sd) == 21
    call, keep = _wgan(wgan_sd, n_tensors=20)
    _refuses(call, 'sbc_wgan_create', 'a generator with 1 extra layers has 21 float tensors (got 20)')


def test_score_create_refuses_a_missing_weight(weights64):
    sd = dict(weights64[1])
    del sd['res2.0.conv2.conv.weight']
    call, keep = _score(sd)
    _refuses(call, 'sbc_score_create', 'res2.0.conv2.conv.weight')


def test_score_create_refuses_a_norm_of_the_wrong_size(weights64):
    call, keep = _score(dict(weights64[1], **{'normalizer.alpha': np.zeros(5)}))
    _refuses(call, 'sbc_score_create', 'normalizer.alpha', '5 elements', 'expected 32')


def test_score_create_refuses_fused_res_blocks_outside_f16x2(weights64):
    call, keep = _score(weights64[1], conv_mode=0, flags=4)
    _refuses(call, 'sbc_score_create', 'SBC_SCORE_FUSE_RES needs conv_mode 3')


@pytest.mark.parametrize('edit', [_no_name, _no_data], ids=['name', 'data'])
@pytest.mark.parametrize('which', ['ldamp', 'wgan', 'score'])
def test_create_refuses_a_ref_without_name_or_data(which, edit, ldamp_sd, wgan_sd, weights64):
    if which == 'ldamp':
        call, keep = _ldamp(ldamp_sd, edit=edit)
    elif which == 'wgan':
        call, keep = _wgan(wgan_sd, edit=edit)
    else:
        call, keep = _score(weights64[1], edit=edit)
    _refuses(call, 'sbc_%s_create' % which, 'tensor 1', 'no name', 'data')
