from .optimizers import (SGD, Adadelta, Adagrad, Adam, Adamax, KVariable, Nadam, Optimizer, RMSprop, deserialize,
                         get, get_value, serialize, set_value)

__all__ = ["SGD", "RMSprop", "Adagrad", "Adadelta", "Adam", "Adamax", "Nadam", "Optimizer", "KVariable", "get",
           "get_value", "set_value", "serialize", "deserialize"]
