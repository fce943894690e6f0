"""MNIST training CLI with the FoM protocol -- the evaluator command of the Cray MNIST
genetic search (``python train.py --epochs N``, ``CrayHPO_mnist.ipynb:75-76``; that
script is referenced but absent from the reference repo).  Flags follow the search space
of ``CrayHPO_mnist.ipynb:41-45`` (``--h1 --h2 --h3 --dropout --optimizer``); prints
``FoM: <min val_loss>`` (lower is better).  Data-parallel under torchrun like train_rpv.
"""
from __future__ import annotations

import argparse
import sys


def build_parser():
    p = argparse.ArgumentParser(description="MNIST CNN training (FoM protocol)")
    p.add_argument("--epochs", type=int, default=4)
    p.add_argument("--h1", type=int, default=4)
    p.add_argument("--h2", type=int, default=8)
    p.add_argument("--h3", type=int, default=16)
    p.add_argument("--dropout", type=float, default=0.2)
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
                   help="a Keras loss name in categorical_crossentropy's place (mse, mae, msle, logcosh, hinge, "
                        "squared_hinge, categorical_hinge, kld, poisson)")
    p.add_argument("--lr", type=float, default=None)
    p.add_argument("--batch-size", type=int, default=128)
    p.add_argument("--valid-frac", type=float, default=0.17)
    p.add_argument("--n-train", type=int, default=60000)
    p.add_argument("--fom", choices=["best", "last"], default="best")
    p.add_argument("--metrics", default=None, help="compile metrics, comma separated: accuracy, auc")
    p.add_argument("--weighted-metrics", default=None,
                   help="compile weighted_metrics, comma separated")
    p.add_argument("--fom-metric", default="val_loss",
                   help="the logged val_ name the FoM line reports (acc and the ROC family print 1 - value)")
    p.add_argument("--verbose", type=int, default=2)
    return p


def main(argv=None):
    a = build_parser().parse_args(argv)
    from ..parallel import hvd
    from .mnist import load_data
    from .zoo import clipped_optimizer, fom_from_history, mnist_cnn, parse_metric_list
    hvd.init()
    x, y, _, _ = load_data(n_train=a.n_train)
    x, y = x[:a.n_train], y[:a.n_train]
    model = mnist_cnn(h1=a.h1, h2=a.h2, h3=a.h3, dropout=a.dropout,
                      optimizer=clipped_optimizer(a.optimizer, a.lr, a.clipnorm, a.clipvalue), lr=a.lr,
                      use_horovod=hvd.size() > 1, l2=a.l2, activation=a.activation, batch_norm=a.batch_norm,
                      pool=a.pool, global_pool=a.global_pool, loss=a.loss, metrics=parse_metric_list(a.metrics),
                      weighted_metrics=parse_metric_list(a.weighted_metrics))
    cbs = []
    if hvd.size() > 1:
        cbs = [hvd.callbacks.BroadcastGlobalVariablesCallback(0), hvd.callbacks.MetricAverageCallback()]
    h = model.fit(x, y, batch_size=a.batch_size, epochs=a.epochs, validation_split=a.valid_frac,
                  verbose=a.verbose if hvd.rank() == 0 else 0, callbacks=cbs)
    print("FoM:", fom_from_history(h.history, a.fom_metric, a.fom))
    sys.stdout.flush()
    hvd.shutdown()
    return h


if __name__ == "__main__":
    main()
