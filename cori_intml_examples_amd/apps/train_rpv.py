"""Distributed RPV classifier training CLI (``train_rpv.py:1-85``): the batch job
(``batch_scripts/train_rpv.sh``) and the HPO evaluator command
(``CrayHPO_rpv.ipynb:145``).  Same flags and defaults as ``train_rpv.py:16-31``; prints
the ``FoM: <float>`` line the HPO evaluators parse (``train_rpv.py:76-79``).

One rank per GPU:

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 \\
        -m cori_intml_examples_amd.apps.train_rpv --lr-scaling linear --fom best

Extra flags (not in the reference): ``--synthetic`` (auto-enabled when ``--input-dir``
has no ``train.h5``: synthetic events of the RPV schema), ``--channels``, ``--seed``,
``--verbose``, ``--metrics`` / ``--weighted-metrics`` (compile's lists: auc, purity, efficiency on the device),
``--fom-metric`` (which logged ``val_`` name the FoM line reports), ``--use-weights`` (the per-event weights as ``sample_weight`` of the training
and validation loss; default off), ``--shard`` / ``--replicate`` (data-parallel sampling: each rank reads a
disjoint shard, or -- the reference's semantics -- the full dataset with its own shuffle).
"""
from __future__ import annotations

import argparse
import os
import socket
import sys


def build_parser():
    p = argparse.ArgumentParser(description="RPV calorimeter-image CNN: data-parallel training on MI355X "
                                            "(one rank per GPU), prints the HPO figure of merit")
    # no site-specific default: $RPV_DATA_DIR, else ./data/atlas-rpv-images (synthetic if absent)
    p.add_argument("--input-dir", default=os.environ.get("RPV_DATA_DIR", os.path.join("data", "atlas-rpv-images")))
    p.add_argument("--n-train", type=int, default=64000)
    p.add_argument("--n-valid", type=int, default=32000)
    p.add_argument("--n-test", type=int, default=0)
    p.add_argument("--h1", type=int, default=16)
    p.add_argument("--h2", type=int, default=32)
    p.add_argument("--h3", type=int, default=64)
    p.add_argument("--h4", type=int, default=128)
    p.add_argument("--dropout", type=float, default=0.2)
    p.add_argument("--lr", type=float, default=0.001)
    p.add_argument("--lr-scaling", choices=["linear"])
    p.add_argument("--optimizer", default="Adam")
    p.add_argument("--clipnorm", type=float, default=None, help="Keras clipnorm: clip by the global gradient norm")
    p.add_argument("--clipvalue", type=float, default=None, help="Keras clipvalue: clamp every gradient element")
    p.add_argument("--l2", type=float, default=0.0, help="l2 kernel regularizer on every Conv2D / Dense (0: none)")
    p.add_argument("--activation", default="relu",
                   help="hidden activation of every Conv2D / Dense: relu, tanh, sigmoid, hard_sigmoid, elu, selu, "
                        "softplus, softsign")
    p.add_argument("--batch-norm", action="store_true",
                   help="a BatchNormalization between every hidden Conv2D / Dense and its activation")
    p.add_argument("--pool", choices=["max", "avg"], default="max", help="the 2x2 pooling layers: MaxPooling2D or AveragePooling2D")
    p.add_argument("--global-pool", choices=["avg", "max"], default=None,
                   help="a GlobalAveragePooling2D / GlobalMaxPooling2D in the Flatten's place")
    p.add_argument("--loss", default=None, metavar="NAME",
                   help="a Keras loss name in binary_crossentropy's place (mse, mae, msle, logcosh, hinge, "
                        "squared_hinge, categorical_hinge, kld, poisson)")
    p.add_argument("--batch-size", type=int, default=64)
    p.add_argument("--n-epochs", type=int, default=4)
    p.add_argument("--fom", choices=["best", "last"])
    # extensions
    p.add_argument("--synthetic", action="store_true")
    p.add_argument("--channels", type=int, default=1)
    p.add_argument("--seed", type=int, default=None)
    p.add_argument("--verbose", type=int, default=2)
    p.add_argument("--use-weights", action="store_true",
                   help="weight the training and validation loss by the per-event weights")
    p.add_argument("--metrics", default=None, help="compile metrics, comma separated: accuracy, auc, purity, efficiency")
    p.add_argument("--weighted-metrics", default=None,
                   help="compile weighted_metrics, comma separated (needs --use-weights)")
    p.add_argument("--fom-metric", default="val_loss",
                   help="the logged val_ name the FoM line reports (acc and the ROC family print 1 - value)")
    g = p.add_mutually_exclusive_group()
    g.add_argument("--shard", dest="shard", action="store_true", default=None)
    g.add_argument("--replicate", dest="shard", action="store_false")
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.weighted_metrics and not args.use_weights:
        parser.error("--weighted-metrics needs --use-weights")
    from ..parallel import hvd
    from ..utils import set_random_seed
    from .rpv import build_model, load_dataset, train_model
    from .zoo import clipped_optimizer, fom_from_history, parse_metric_list

    st = hvd.init(shard_data=args.shard)
    print("[train_rpv] rank %d/%d (local %d) on %s, data plane %s" % (
        hvd.rank(), hvd.size(), hvd.local_rank(), socket.gethostname(),
        st.plane or ("rccl" if st.comm is not None else st.backend)))
    if args.seed is not None:
        set_random_seed(args.seed + hvd.rank())

    synthetic = args.synthetic or not os.path.exists(os.path.join(args.input_dir, "train.h5"))
    if synthetic and not args.synthetic:
        print("input dir %s has no train.h5: using synthetic RPV events" % args.input_dir)
    train_data, valid_data, test_data = load_dataset(args.input_dir, args.n_train, args.n_valid, args.n_test,
                                                     synthetic=synthetic, channels=args.channels)
    train_input, train_labels, train_weights = train_data
    valid_input, valid_labels, valid_weights = valid_data
    test_input, test_labels, _ = test_data
    print("train shape:", train_input.shape, "Mean label:", train_labels.mean())
    print("valid shape:", valid_input.shape, "Mean label:", valid_labels.mean())
    if args.n_test > 0:
        print("test shape: ", test_input.shape, "Mean label:", test_labels.mean())

    lr = args.lr * hvd.size() if args.lr_scaling == "linear" else args.lr
    model = build_model(train_input.shape[1:], conv_sizes=[args.h1, args.h2, args.h3], fc_sizes=[args.h4],
                        dropout=args.dropout,
                        optimizer=clipped_optimizer(args.optimizer, lr, args.clipnorm, args.clipvalue), lr=lr,
                        use_horovod=True, l2=args.l2, activation=args.activation,
                        batch_norm=args.batch_norm, pool=args.pool, global_pool=args.global_pool, loss=args.loss,
                        metrics=parse_metric_list(args.metrics),
                        weighted_metrics=parse_metric_list(args.weighted_metrics))
    if hvd.rank() == 0:
        model.summary()

    print("[train_rpv] %d epochs, batch %d per rank, lr %g" % (args.n_epochs, args.batch_size, lr))
    history = train_model(model, train_input=train_input, train_labels=train_labels, valid_input=valid_input,
                          valid_labels=valid_labels, batch_size=args.batch_size, n_epochs=args.n_epochs,
                          verbose=args.verbose, use_horovod=True,
                          train_weights=train_weights if args.use_weights else None,
                          valid_weights=valid_weights if args.use_weights else None)
    if hvd.rank() == 0 and getattr(history, "data_plane", None):
        print("[train_rpv] gradient reducer %s" % history.data_plane)
    if args.fom in ("best", "last"):
        # one write per line: the ranks share the launcher's pipe, and print's separate writes
        # of "FoM:" and the value interleave across ranks
        sys.stdout.write("FoM: %s\n" % fom_from_history(history.history, args.fom_metric, args.fom))
        sys.stdout.flush()
    sys.stdout.flush()

    if hvd.rank() == 0 and args.n_test > 0:
        score = model.evaluate(test_input, test_labels, verbose=2)
        print("Test loss:", score[0])
        print("Test accuracy:", score[1])
    hvd.shutdown()
    return history


if __name__ == "__main__":
    main()
