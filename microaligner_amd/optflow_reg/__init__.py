from .flow_calc import TileFlowCalc, farneback
from .optflow_registrator import OptFlowRegistrator, compose_flows, merge_two_flows
from .warper import Warper
