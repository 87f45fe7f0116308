"""CPU half of the suite for the grouped template match (cbh_template_match_pairs): the fixture of
tests/template_pairs_rules.py is hard enough on the model, the model of a pair is the chain's model of that template and
that one candidate, and the Python entry refuses what it cannot send."""
import numpy as np
import pytest

import template_images_rules as M
import template_pairs_rules as P


@pytest.mark.parametrize("ch", [1, 3, 4])
def test_fixture_conditions_hold_on_the_model(ch):
    images, pt, pc, model = P.pairs_fixture(ch)
    assert len(model) == len(P.PAIRS) and all(m is not None for m in model)
    assert P.pairs_conditions(images, pt, pc, model) == []
    th, tw = images[P.CROP].shape[:2]
    assert (tw, th) == (P.CROP_W, P.CROP_H) and images[P.THIN].shape[:2] == (8, 3000)
    assert model[P.PAIRS.index((P.TMPL, P.THIN))]["status"] == M.EMPTY_RESIZE
    assert model[P.PAIRS.index((P.TMPL, P.TMPL))]["r"]["score"] == 0


def test_conditions_notice_an_easy_fixture():
    images, pt, pc, model = P.pairs_fixture(1)
    keep = [p for p in range(len(pt)) if pt[p] == P.TMPL and pc[p] != P.THIN]
    bad = P.pairs_conditions(images, pt[keep], pc[keep], [model[p] for p in keep])
    for what in ("fewer than three template sizes", "no flat template with two pairs", "no empty resize",
                 "no template with exactly one pair", "every template's pairs are adjacent", "no (A, B) with its (B, A)"):
        assert what in bad


def test_a_pair_is_the_chain_of_its_template_and_its_candidate():
    images, pt, pc, model = P.pairs_fixture(3)
    for p in (P.PAIRS.index((P.SHIFTED, P.TMPL)), P.PAIRS.index((P.CROP, P.TMPL)), P.PAIRS.index((P.FLAT, P.COPY))):
        one = M.template_match_images(images[pt[p]], [images[pc[p]]])[0]
        assert one["status"] == model[p]["status"] and (one["w"], one["h"]) == (model[p]["w"], model[p]["h"])
        assert one["n_keypoints"] == model[p]["n_keypoints"] and one["n_matches"] == model[p]["n_matches"]
        if one["r"] is not None:
            assert one["r"]["score"] == model[p]["r"]["score"] and (one["r"]["m"] == model[p]["r"]["m"]).all()


def test_python_entry_checks_its_arguments_before_the_device():
    from cbird_amd.hashing import TEMPLATE_IMAGE_RESULT_DTYPE, template_match_pairs

    images = P.pairs_images(3)
    res = template_match_pairs(images, [], [])  # nothing to do: nothing is read
    assert res.dtype == TEMPLATE_IMAGE_RESULT_DTYPE and len(res) == 0
    with pytest.raises(ValueError):
        template_match_pairs(images, [0, 1], [0])
    with pytest.raises(ValueError):
        template_match_pairs(images, [len(images)], [0])
    with pytest.raises(ValueError):
        template_match_pairs(images + [np.zeros((4, 4), np.uint8)], [0], [1])
