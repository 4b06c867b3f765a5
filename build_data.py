#!/usr/bin/env python
"""Drop-in for the reference's ``python build_data.py --aug N`` (build_data.py:290-295): builds the GTSDB detector sets with the
params of experiments/darknet_r/params.json, every pixel on the device (capsyolo_amd/build_data.py).  New, optional:
  --root DIR      the GTSDB root (raw_GTSDB/ inside it; default data/GTSDB)
  --gtsrb DIR     the GTSRB root: the signs that --aug pastes, and what --gtsrb_set builds (default data/GTSRB)
  --seed S        the shuffle and the augmentation's randomness (default 0, the reference's np.random.seed(0))
  --keep_raw      also write train_raw.p, the raw training frames and boxes that ``main.py --augment`` pastes over on line
  --gtsrb_set     build the GTSRB classifier sets too (the reference's commented-out gtsrb() call)
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import capsyolo_amd  # noqa: E402,F401
from capsyolo_amd import build_data, config, utils  # noqa: E402

parser = argparse.ArgumentParser()
parser.add_argument('--aug', default=0, type=int, help=' need data augmentation?')
parser.add_argument('--root', default=config.GTSDB, help='GTSDB root')
parser.add_argument('--gtsrb', default=config.GTSRB, help='GTSRB root')
parser.add_argument('--seed', default=0, type=int, help='random seed')
parser.add_argument('--keep_raw', action='store_true', help='also write train_raw.p for main.py --augment')
parser.add_argument('--gtsrb_set', action='store_true', help='also build the GTSRB train/eval/test sets')


def main(argv=None):
    args = parser.parse_args(argv)
    if args.gtsrb_set:
        build_data.gtsrb(args.gtsrb, seed=args.seed)
    params = utils.Params(os.path.join(ROOT, 'experiments', 'darknet_r', 'params.json'))
    return build_data.gtsdb(params, aug_size=args.aug, root=args.root, gtsrb_root=args.gtsrb, seed=args.seed,
                            keep_raw=args.keep_raw)


if __name__ == '__main__':
    main()
