"""Generate tests/golden/reference_cards.json -- the data fields of the reference's asset cards
(`sonar/cards/*.yaml` of facebookresearch/SONAR v0.4.0) that sonar_amd/cards.py and sonar_amd/nllb_langs.py
restate: every card's `name`, `checkpoint` and `tokenizer` URL, and the `langs` list of
text_sonar_basic_encoder.yaml (the order of the NLLB language tokens).  The fixture lets
tests/test_host_cpu.py and tests/test_pipeline_cpu.py check those tables without a reference checkout.

Usage:  python tests/golden/make_golden_cards.py <path of a facebookresearch/SONAR checkout>
"""
import json
import os
import sys

import yaml

CARDS = ("text_sonar_basic_encoder.yaml", "text_sonar_basic_decoder.yaml", "text_sonar_finetuned_decoder.yaml",
         "sonar_speech_encoder.yaml", "sonar_mutox.yaml")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_cards.json")


def main(ref_root: str) -> None:
    out = {"cards": {}, "text_sonar_basic_encoder_langs": None}
    for f in CARDS:
        with open(os.path.join(ref_root, "sonar", "cards", f)) as fh:
            docs = list(yaml.safe_load_all(fh))
        out["cards"][f] = [{k: d[k] for k in ("name", "checkpoint", "tokenizer") if k in d} for d in docs if d]
        if f == "text_sonar_basic_encoder.yaml":
            out["text_sonar_basic_encoder_langs"] = docs[0]["langs"]
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", OUT, sum(len(v) for v in out["cards"].values()), "cards")


if __name__ == "__main__":
    main(sys.argv[1])
