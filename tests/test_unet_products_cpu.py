"""The binding and the arguments of the fine-tuned encoder's product modes (said_amd/csrc/said_unet_train_products.h), without a GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_matches_its_header():
    """tests/test_host_cpu.py's check of a binding group against its headers, for the "unet_products" group of _engine.added_groups()."""
    import test_host_cpu as th
    from said_amd import _engine
    lib, g = _engine.load_library("unet_products"), _engine.added_groups()["unet_products"]
    assert g.headers == ("said_amd/csrc/said_unet_train_products.h",)
    declared = {name: sig for h in g.headers for name, sig in th._declarations(th._header(h)).items()}
    assert set(declared) == set(g.table) and len(declared) == 3
    others = [o for o in _engine.ABI.values()] + [o for k, o in _engine.added_groups().items() if k != "unet_products"]
    assert not [name for o in others for name in o.table if name in declared], "bound by two groups"
    assert [name for name in declared if not hasattr(lib, name)] == [], "declared but not exported"
    assert th._mismatches(declared, g.table) == []
    assert all(getattr(lib, name).argtypes == sig[1] for name, sig in g.table.items())
    enums = th._enums(th._header(g.headers[0]))
    assert enums["SAID_UT_PRODUCTS_FP32"] == 0 and enums["SAID_UT_PRODUCTS_SPLIT_F16"] == 1
    assert _engine.ENCODER_PRODUCTS.index("fp32") == enums["SAID_UT_PRODUCTS_FP32"]
    assert _engine.ENCODER_PRODUCTS.index("split_fp16") == enums["SAID_UT_PRODUCTS_SPLIT_F16"] and len(_engine.ENCODER_PRODUCTS) == 2
    assert [enums[k] for k in ("SAID_UT_PRODUCT_FORWARD", "SAID_UT_PRODUCT_DGRAD", "SAID_UT_PRODUCT_WGRAD")] == [0, 1, 2]
    assert lib.said_unet_train_encoder_products(None) == -1 and lib.said_unet_train_set_encoder_products(None, 1) == -1


def test_trainer_refuses_the_argument_without_finetuning():
    """Before any device is looked at."""
    from said_amd.training import UNetTrainer
    for mode in ("fp32", "split_fp16"):
        with pytest.raises(ValueError, match="encoder_products: the encoder is frozen"):
            UNetTrainer({}, "cpu", encoder_products=mode)
    with pytest.raises(ValueError, match="encoder_products must be one of"):
        UNetTrainer({}, "cpu", finetune_audio_layers=2, encoder_products="bf16")


def test_cli_argument():
    sys.path.insert(0, os.path.join(ROOT, "script"))
    try:
        import train
    finally:
        sys.path.pop(0)
    ap = train.build_parser()
    assert ap.parse_args([]).encoder_products is None
    assert ap.parse_args(["--finetune_audio_encoder", "--encoder_products", "split_fp16"]).encoder_products == "split_fp16"
    with pytest.raises(SystemExit):
        ap.parse_args(["--encoder_products", "bf16"])
    with pytest.raises(SystemExit, match="needs --finetune_audio_encoder"):
        train.main(["--encoder_products", "split_fp16"])
