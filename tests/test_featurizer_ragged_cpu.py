"""Host-side surface of the ragged mel path (no GPU): the reference's two positional arguments of extract_features stay in front of
the batch_size keyword, and the binding of the new entry point has the argument list of include/vpmi.h."""
import inspect
import os
import re


def test_extract_features_keeps_the_reference_arguments_in_front():
    from ppvector.trainer import PPVectorTrainer
    p = inspect.signature(PPVectorTrainer.extract_features).parameters
    assert list(p) == ['self', 'save_dir', 'max_duration', 'batch_size']
    assert (p['save_dir'].default, p['max_duration'].default, p['batch_size'].default) == ('dataset/features', 100, 1)


def test_ragged_mel_binding_matches_the_header():
    from ppvector import _native as N
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'vpmi.h'), encoding='utf-8').read()
    decl = re.search(r'int vp_melspec_cmn_ragged_f32\((.*?)\);', header, re.S).group(1)
    res, args = N._PROTOS['vp_melspec_cmn_ragged_f32']
    assert res is N.c_int and len(args) == len(decl.split(',')) == 12
    # same shape as the Fbank entry point it is modelled on, with the mel options
    _, fb = N._PROTOS['vp_fbank_cmn_ragged_f32']
    assert [a for a in args if a is not args[5]] == [a for a in fb if a is not fb[5]] and args[5]._type_ is N.MelOpts
