"""``MODE=<train|basis|synthesize|test|publish|preprocess|evaluation> python -m fastvocoder_amd.bin.launcher --flags``
-- the reference's $MODE dispatch (bin/launcher.py:7-19): training (HiFi-GAN and
Multiband-HiFi-GAN), learning Basis-MelGAN's basis and target weights, the inference-side modes, the dataset
preparation and the evaluation."""
import os
import sys


def main():
    mode = os.getenv("MODE")
    if mode == "synthesize":
        from .synthesize import run_synthesizer
        run_synthesizer()
    elif mode == "test":
        from .test import run_test
        run_test()
    elif mode == "publish":
        from .publish import run_publisher
        run_publisher()
    elif mode == "preprocess":
        from .preprocess import run_preprocess
        run_preprocess()
    elif mode == "evaluation":
        from .evaluation import run_evaluation
        run_evaluation()
    elif mode == "train":
        from .train import run_train
        run_train()
    elif mode == "basis":
        from .basis import run_basis
        run_basis()
    else:
        sys.exit("set MODE=train | basis | synthesize | test | publish | preprocess | evaluation")


if __name__ == "__main__":
    main()
